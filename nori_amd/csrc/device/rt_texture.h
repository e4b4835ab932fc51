/*
 * rt_texture.h -- albedo textures of diffuse BSDFs (include/nori_hip.h, nori_texture_desc).
 *
 * The reference has no Texture class; what it pins is the coordinate a texture is looked up at: its.uv, the mesh's
 * interpolated texture coordinates or the barycentric (u, v) where it has none (src/accel.cpp:38,73-77; hit_uv below, which
 * surface_fill and the shading share).  The lookup is stated in the header to the last operation, float32 without FMA
 * contraction (-ffp-contract=off), so that a numpy float32 restatement reproduces it bit for bit (tests/test_gpu_textures.py).
 * The texture unit's sampler is not used: its filter weights are fixed-point and cannot be restated on a CPU.
 *
 * Storage: the texels of every image texture in one array of 16-B RGBA records (a texel is one dwordx4 load; A unused), and
 * a table of TexRec records, one per texture, index = nori_mesh_desc::albedo_texture - 1 (MeshRec::pad[0] holds the 1-based
 * index of a textured mesh, kMeshTextured its flag).
 */
#pragma once
#include "rt_types.h"

namespace nrt {

constexpr uint32_t kTexImage = 0u, kTexChecker = 1u;
constexpr uint32_t kTexMaxDim = 16384u;

struct TexRec {                /* 48 B */
    uint32_t type;             /* kTexImage / kTexChecker */
    uint32_t width, height;
    uint32_t texel_offset;     /* first texel in DevScene::texels */
    float uscale, vscale, uoffset, voffset;
    float color0[3];
    uint32_t bilinear;         /* nori_texture_filter: 1 = bilinear */
    float color1[3];
    uint32_t clamp;            /* nori_texture_wrap: 1 = clamp */
};

NORI_HD float tex_lerp(float a, float b, float f) { return a + f * (b - a); }

/* wrap of a coordinate already scaled and offset; returns it in [0, 1] */
NORI_HD float tex_wrap(float s, bool clamp) {
    if (clamp) return fminf(fmaxf(s, 0.0f), 1.0f);
    return s - floorf(s);
}
NORI_HD int tex_index(int i, int n, bool clamp) {
    if (clamp) return i < 0 ? 0 : (i > n - 1 ? n - 1 : i);
    i %= n;
    return i < 0 ? i + n : i;
}

NORI_HD f3 texel_rgb(const f4 *texels, uint32_t off, int w, int i, int j) {
    return xyz(texels[off + (uint32_t) j * (uint32_t) w + (uint32_t) i]);
}

/* the albedo of texture `t` at texture coordinates uv (include/nori_hip.h states each step) */
NORI_HD f3 texture_lookup(const TexRec &t, const f4 *texels, f2 uv) {
    float s = uv.x * t.uscale + t.uoffset, r = uv.y * t.vscale + t.voffset;
    if (!(fabsf(s) < kInf)) s = 0.0f;
    if (!(fabsf(r) < kInf)) r = 0.0f;
    if (t.type == kTexChecker) {
        const float ps = floorf(s) - 2.0f * floorf(s * 0.5f), pt = floorf(r) - 2.0f * floorf(r * 0.5f);
        return ps == pt ? mk3(t.color0[0], t.color0[1], t.color0[2]) : mk3(t.color1[0], t.color1[1], t.color1[2]);
    }
    const bool clamp = t.clamp != 0u;
    const int w = (int) t.width, h = (int) t.height;
    s = tex_wrap(s, clamp);
    r = 1.0f - tex_wrap(r, clamp);
    if (!t.bilinear) {
        int i = (int) (s * (float) w), j = (int) (r * (float) h);
        i = i < w - 1 ? i : w - 1; j = j < h - 1 ? j : h - 1;
        return texel_rgb(texels, t.texel_offset, w, i, j);
    }
    const float x = s * (float) w - 0.5f, y = r * (float) h - 0.5f;
    const float x0 = floorf(x), y0 = floorf(y);
    const float fx = x - x0, fy = y - y0;
    const int i0 = tex_index((int) x0, w, clamp), i1 = tex_index((int) x0 + 1, w, clamp);
    const int j0 = tex_index((int) y0, h, clamp), j1 = tex_index((int) y0 + 1, h, clamp);
    const f3 a = texel_rgb(texels, t.texel_offset, w, i0, j0), b = texel_rgb(texels, t.texel_offset, w, i1, j0);
    const f3 c = texel_rgb(texels, t.texel_offset, w, i0, j1), d = texel_rgb(texels, t.texel_offset, w, i1, j1);
    const f3 top = mk3(tex_lerp(a.x, b.x, fx), tex_lerp(a.y, b.y, fx), tex_lerp(a.z, b.z, fx));
    const f3 bot = mk3(tex_lerp(c.x, d.x, fx), tex_lerp(c.y, d.y, fx), tex_lerp(c.z, d.z, fx));
    return mk3(tex_lerp(top.x, bot.x, fy), tex_lerp(top.y, bot.y, fy), tex_lerp(top.z, bot.z, fy));
}

} // namespace nrt
