"""The XML surface of albedo textures (nori_amd/csrc/host/texture.cpp): <texture type="image|checkerboard" name="albedo"> under a
diffuse BSDF, PNG and OpenEXR files decoded into the descriptor bit for bit as numpy decodes them (sRGB table included), and
the parse errors."""
from __future__ import annotations

import os
import struct
import zlib

import numpy as np
import pytest

from nori_amd import host
from nori_amd._capi import NoriError

F = np.float32


def srgb_table():
    """the 256-entry sRGB decoding table: IEC 61966-2-1 in double, rounded to float"""
    c = np.arange(256, dtype=np.float64) / 255.0
    return np.where(c <= 0.04045, c / 12.92, ((c + 0.055) / 1.055) ** 2.4).astype(F)


def write_png(path, px, color_type, filters=(0, 1, 2, 3, 4), interlace=0, depth=8):
    """8-bit PNG of px (H, W, channels uint8), one scanline filter per row in turn (None, Sub, Up, Average, Paeth)"""
    h, w, ch = px.shape
    raw, prev = b"", np.zeros(w * ch, np.int32)
    for y in range(h):
        row = px[y].reshape(-1).astype(np.int32)
        f = filters[y % len(filters)]
        out = np.zeros_like(row)
        for x in range(w * ch):
            a = row[x - ch] if x >= ch else 0
            b = prev[x]
            c = prev[x - ch] if x >= ch else 0
            if f == 0: pred = 0
            elif f == 1: pred = a
            elif f == 2: pred = b
            elif f == 3: pred = (a + b) // 2
            else:
                p = a + b - c
                pa, pb, pc = abs(p - a), abs(p - b), abs(p - c)
                pred = a if (pa <= pb and pa <= pc) else (b if pb <= pc else c)
            out[x] = (row[x] - pred) & 0xFF
        raw += bytes([f]) + out.astype(np.uint8).tobytes()
        prev = row

    def chunk(t, d):
        return struct.pack(">I", len(d)) + t + d + struct.pack(">I", zlib.crc32(t + d) & 0xFFFFFFFF)
    data = b"\x89PNG\r\n\x1a\n" + chunk(b"IHDR", struct.pack(">IIBBBBB", w, h, depth, color_type, 0, 0, interlace))
    z = zlib.compress(raw)
    data += chunk(b"IDAT", z[:len(z) // 2]) + chunk(b"IDAT", z[len(z) // 2:]) + chunk(b"IEND", b"")
    open(path, "wb").write(data)


SCENE = """<scene><integrator type="path_mis"/>
  <sampler type="independent"><integer name="sampleCount" value="4"/></sampler>
  <camera type="perspective"><float name="fov" value="60"/><integer name="width" value="24"/><integer name="height" value="16"/>
    <transform name="toWorld"><lookat origin="0,1.5,1.5" target="0,0,0" up="0,1,0"/></transform></camera>
  {meshes}
  <mesh type="obj"><string name="filename" value="light.obj"/>
    <emitter type="area"><color name="radiance" value="5, 5, 5"/></emitter></mesh>
</scene>"""


def write_objs(d):
    (d / "quad.obj").write_text("v -1 0 -1\nv 1 0 -1\nv 1 0 1\nv -1 0 1\nvt 0 0\nvt 1 0\nvt 1 1\nvt 0 1\nf 1/1 3/3 2/2\nf 1/1 4/4 3/3\n")
    (d / "light.obj").write_text("v -0.3 1.5 -0.3\nv 0.3 1.5 -0.3\nv 0.3 1.5 0.3\nv -0.3 1.5 0.3\nf 1 2 3\nf 1 3 4\n")


def mesh(bsdf):
    return f'<mesh type="obj"><string name="filename" value="quad.obj"/>{bsdf}</mesh>'


def test_xml_textures_load_into_the_descriptor(tmp_path):
    write_objs(tmp_path)
    rng = np.random.default_rng(5)
    imgs = {"rgb.png": (rng.integers(0, 256, (5, 7, 3), dtype=np.uint8), 2), "rgba.png": (rng.integers(0, 256, (6, 4, 4), dtype=np.uint8), 6),
            "gray.png": (rng.integers(0, 256, (3, 9, 1), dtype=np.uint8), 0), "graya.png": (rng.integers(0, 256, (4, 3, 2), dtype=np.uint8), 4)}
    for name, (px, ct) in imgs.items():
        write_png(str(tmp_path / name), px, ct)
    exr = rng.uniform(0, 2, (6, 5, 3)).astype(F)
    exr[0, 0] = [0.0, 1.0, 0.5]
    host.save_images(str(tmp_path / "lin"), exr)          # writes lin.exr (and lin.png)
    os.makedirs(tmp_path / "tex", exist_ok=True)
    os.replace(tmp_path / "lin.exr", tmp_path / "tex" / "lin.exr")
    meshes = [
        mesh('<bsdf type="diffuse"><texture type="image" name="albedo"><string name="filename" value="rgb.png"/>'
             '<string name="filter" value="nearest"/><string name="wrap" value="clamp"/><float name="uscale" value="4"/>'
             '<float name="vscale" value="2"/><float name="uoffset" value="0.25"/><float name="voffset" value="-0.5"/></texture></bsdf>'),
        mesh('<bsdf type="diffuse"><texture type="image"><string name="filename" value="rgba.png"/></texture></bsdf>'),
        mesh('<bsdf type="diffuse"><texture type="image" name="albedo"><string name="filename" value="gray.png"/>'
             '<boolean name="srgb" value="false"/></texture></bsdf>'),
        mesh('<bsdf type="diffuse"><texture type="image" name="albedo"><string name="filename" value="graya.png"/></texture></bsdf>'),
        mesh('<bsdf type="diffuse"><texture type="image" name="albedo"><string name="filename" value="tex/lin.exr"/></texture></bsdf>'),
        mesh('<bsdf type="diffuse"><texture type="image" name="albedo"><string name="filename" value="tex/lin.exr"/>'
             '<boolean name="srgb" value="true"/></texture></bsdf>'),
        mesh('<bsdf type="diffuse"><texture type="checkerboard" name="albedo"><color name="color0" value="0.9, 0.1, 0.2"/>'
             '<color name="color1" value="0.05, 0.6, 0.3"/><float name="uscale" value="8"/><float name="vscale" value="8"/></texture></bsdf>'),
        mesh('<bsdf type="diffuse"><color name="albedo" value="0.3, 0.3, 0.3"/></bsdf>'),
    ]
    (tmp_path / "s.xml").write_text(SCENE.format(meshes="\n  ".join(meshes)))
    sc = host.load_xml(str(tmp_path / "s.xml"))
    assert [m.albedo_texture for m in sc.meshes] == [0, 1, 2, 3, 4, 5, 6, None, None]
    assert len(sc.textures) == 7
    tab = srgb_table()
    t = sc.textures
    assert np.array_equal(t[0].texels, tab[imgs["rgb.png"][0]])
    assert (t[0].filter, t[0].wrap, t[0].uscale, t[0].vscale, t[0].uoffset, t[0].voffset) == ("nearest", "clamp", 4.0, 2.0, 0.25, -0.5)
    assert np.array_equal(t[1].texels, tab[imgs["rgba.png"][0][..., :3]])          # alpha ignored
    assert (t[1].filter, t[1].wrap, t[1].uscale) == ("bilinear", "repeat", 1.0)      # the defaults
    g = imgs["gray.png"][0]
    assert np.array_equal(t[2].texels, np.repeat((g.astype(np.float64) / 255.0).astype(F), 3, axis=2))
    assert np.array_equal(t[3].texels, np.repeat(tab[imgs["graya.png"][0][..., :1]], 3, axis=2))
    assert np.array_equal(t[4].texels, exr)                                          # OpenEXR: linear unless told otherwise
    e = exr.astype(np.float64)
    assert np.array_equal(t[5].texels, np.where(e <= 0.04045, e / 12.92, ((e + 0.055) / 1.055) ** 2.4).astype(F))
    assert t[6].kind == "checkerboard" and t[6].texels is None and t[6].uscale == 8.0
    assert t[6].color0 == tuple(F([0.9, 0.1, 0.2])) and t[6].color1 == tuple(F([0.05, 0.6, 0.3]))
    # row 0 of the texels is the top row of the file
    assert np.array_equal(t[0].texels[0], tab[imgs["rgb.png"][0][0]])


@pytest.mark.parametrize("bsdf,msg", [
    ('<bsdf type="mirror"><texture type="checkerboard" name="albedo"/></bsdf>', "only be the albedo of a diffuse BSDF, not of Mirror"),
    ('<bsdf type="dielectric"><texture type="checkerboard" name="albedo"/></bsdf>', "not of Dielectric"),
    ('<bsdf type="microfacet"><texture type="checkerboard" name="albedo"/></bsdf>', "not of Microfacet"),
    ('<bsdf type="diffuse"><color name="albedo" value="0.5, 0.5, 0.5"/><texture type="checkerboard" name="albedo"/></bsdf>',
     "both an albedo color and an albedo texture"),
    ('<bsdf type="diffuse"><texture type="checkerboard" name="albedo"/><texture type="checkerboard" name="albedo"/></bsdf>', "only have one albedo texture"),
    ('<bsdf type="diffuse"><texture type="checkerboard" name="kd"/></bsdf>', 'can only be named "albedo"'),
    ('<bsdf type="diffuse"><texture type="image" name="albedo"><string name="filename" value="missing.png"/></texture></bsdf>',
     'cannot read image'),
    ('<bsdf type="diffuse"><texture type="image" name="albedo"><string name="filename" value="missing.exr"/></texture></bsdf>',
     'cannot read image'),
    ('<bsdf type="diffuse"><texture type="image" name="albedo"><string name="filename" value="quad.obj"/></texture></bsdf>',
     "unsupported image"),
    ('<bsdf type="diffuse"><texture type="image" name="albedo"><string name="filename" value="bad16.png"/></texture></bsdf>',
     "unsupported PNG bit depth 16"),
    ('<bsdf type="diffuse"><texture type="image" name="albedo"><string name="filename" value="palette.png"/></texture></bsdf>',
     "unsupported PNG colour type 3"),
    ('<bsdf type="diffuse"><texture type="image" name="albedo"><string name="filename" value="interlaced.png"/></texture></bsdf>',
     "interlaced PNG"),
    ('<bsdf type="diffuse"><texture type="image" name="albedo"><string name="filename" value="notpng.png"/></texture></bsdf>',
     "is not a PNG file"),
    ('<bsdf type="diffuse"><texture type="checkerboard" name="albedo"><string name="filter" value="cubic"/></texture></bsdf>',
     'unknown filter'),
])
def test_xml_texture_errors(tmp_path, bsdf, msg):
    write_objs(tmp_path)
    write_png(str(tmp_path / "bad16.png"), np.zeros((2, 2, 3), np.uint8), 2, depth=16)
    write_png(str(tmp_path / "palette.png"), np.zeros((2, 2, 1), np.uint8), 3)
    write_png(str(tmp_path / "interlaced.png"), np.zeros((2, 2, 3), np.uint8), 2, interlace=1)
    (tmp_path / "notpng.png").write_bytes(b"GIF89a....")
    (tmp_path / "s.xml").write_text(SCENE.format(meshes=mesh(bsdf)))
    with pytest.raises(NoriError, match=msg):
        host.load_xml(str(tmp_path / "s.xml"))


def test_name_is_only_an_attribute_of_texture(tmp_path):
    write_objs(tmp_path)
    (tmp_path / "s.xml").write_text(SCENE.format(meshes=mesh('<bsdf type="diffuse" name="albedo"/>')))
    with pytest.raises(NoriError, match='unexpected attribute "name"'):
        host.load_xml(str(tmp_path / "s.xml"))
