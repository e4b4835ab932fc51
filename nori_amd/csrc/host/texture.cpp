/*
 * texture.cpp -- albedo textures of diffuse BSDFs (an extension: the reference has no Texture class).
 *
 *   <bsdf type="diffuse">
 *     <texture type="image" name="albedo">
 *       <string name="filename" value="wood.png"/>   resolved like <mesh> filenames
 *       <string name="filter" value="bilinear"/>     | nearest
 *       <string name="wrap" value="repeat"/>         | clamp
 *       <boolean name="srgb" value="true"/>          default: true for PNG, false for OpenEXR
 *       <float name="uscale" value="4"/>             vscale, uoffset, voffset
 *     </texture>
 *   </bsdf>
 *   <texture type="checkerboard" name="albedo"> <color name="color0" .../> <color name="color1" .../> scale / offset </texture>
 *
 * Images are decoded to linear RGB floats, row 0 = the top row of the file (nori_texture_desc, include/nori_hip.h, which
 * also states the lookup).  PNG: 8-bit gray, gray + alpha, RGB or RGBA, not interlaced, inflated with zlib; alpha is
 * ignored.  sRGB decoding of 8-bit values goes through a 256-entry table computed in double and rounded to float; float
 * (OpenEXR) values marked sRGB go through the same formula.
 */
#include <nori/bitmap.h>
#include <nori/plugins.h>

#include <zlib.h>

#include <cctype>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <fstream>

NORI_NAMESPACE_BEGIN

namespace {

/* IEC 61966-2-1 decoding, in double */
double srgbToLinear(double c) { return c <= 0.04045 ? c / 12.92 : std::pow((c + 0.055) / 1.055, 2.4); }

const float *srgbTable() {
    static float table[256];
    static bool init = false;
    if (!init) {
        for (int i = 0; i < 256; ++i) table[i] = (float) srgbToLinear(i / 255.0);
        init = true;
    }
    return table;
}

uint32_t be32(const unsigned char *p) { return ((uint32_t) p[0] << 24) | ((uint32_t) p[1] << 16) | ((uint32_t) p[2] << 8) | (uint32_t) p[3]; }

int paeth(int a, int b, int c) {
    const int p = a + b - c, pa = std::abs(p - a), pb = std::abs(p - b), pc = std::abs(p - c);
    return (pa <= pb && pa <= pc) ? a : (pb <= pc ? b : c);
}

/* 8-bit PNG -> width x height x 3 floats (sRGB table or value / 255) */
void loadPNG(const std::string &filename, bool srgb, uint32_t &width, uint32_t &height, std::vector<float> &rgb) {
    std::ifstream is(filename, std::ios::binary);
    if (is.fail()) throw NoriException("cannot read image \"%s\"", filename);
    const std::string f((std::istreambuf_iterator<char>(is)), std::istreambuf_iterator<char>());
    const unsigned char *d = reinterpret_cast<const unsigned char *>(f.data());
    static const unsigned char sig[8] = {137, 80, 78, 71, 13, 10, 26, 10};
    if (f.size() < 8 || std::memcmp(d, sig, 8) != 0) throw NoriException("\"%s\" is not a PNG file", filename);
    size_t i = 8;
    int depth = -1, ctype = -1, interlace = -1;
    std::string idat;
    bool end = false;
    while (!end) {
        if (i + 8 > f.size()) throw NoriException("\"%s\": truncated PNG file", filename);
        const uint32_t len = be32(d + i);
        const std::string type(f, i + 4, 4);
        if (i + 12 + (size_t) len > f.size()) throw NoriException("\"%s\": truncated PNG file", filename);
        const unsigned char *c = d + i + 8;
        if (type == "IHDR") {
            if (len < 13) throw NoriException("\"%s\": bad PNG header", filename);
            width = be32(c); height = be32(c + 4); depth = c[8]; ctype = c[9]; interlace = c[12];
        } else if (type == "IDAT") {
            idat.append(reinterpret_cast<const char *>(c), len);
        } else if (type == "IEND") {
            end = true;
        }
        i += 12 + (size_t) len;
    }
    if (depth < 0) throw NoriException("\"%s\": PNG file without a header", filename);
    int channels = 0;
    switch (ctype) {
    case 0: channels = 1; break;      /* gray */
    case 4: channels = 2; break;      /* gray + alpha */
    case 2: channels = 3; break;      /* RGB */
    case 6: channels = 4; break;      /* RGBA */
    default: throw NoriException("\"%s\": unsupported PNG colour type %d (8-bit gray, gray + alpha, RGB or RGBA only)", filename, ctype);
    }
    if (depth != 8) throw NoriException("\"%s\": unsupported PNG bit depth %d (8 bits per channel only)", filename, depth);
    if (interlace != 0) throw NoriException("\"%s\": interlaced PNG files are not supported", filename);
    if (width == 0 || height == 0 || width > 16384 || height > 16384)
        throw NoriException("\"%s\": PNG of %u x %u pixels (each dimension must be 1 .. 16384)", filename, width, height);
    const size_t stride = (size_t) width * channels;
    std::vector<unsigned char> raw((stride + 1) * height);
    uLongf n = (uLongf) raw.size();
    if (uncompress(raw.data(), &n, reinterpret_cast<const Bytef *>(idat.data()), (uLong) idat.size()) != Z_OK || n != raw.size())
        throw NoriException("\"%s\": corrupt PNG image data", filename);
    std::vector<unsigned char> px(stride * height);
    for (uint32_t y = 0; y < height; ++y) {
        const unsigned char filter = raw[y * (stride + 1)];
        const unsigned char *src = &raw[y * (stride + 1) + 1];
        unsigned char *row = &px[y * stride];
        const unsigned char *up = y > 0 ? &px[(y - 1) * stride] : nullptr;
        for (size_t x = 0; x < stride; ++x) {
            const int a = x >= (size_t) channels ? row[x - channels] : 0, b = up ? up[x] : 0, c = (up && x >= (size_t) channels) ? up[x - channels] : 0;
            int v = src[x];
            switch (filter) {
            case 0: break;
            case 1: v += a; break;
            case 2: v += b; break;
            case 3: v += (a + b) / 2; break;
            case 4: v += paeth(a, b, c); break;
            default: throw NoriException("\"%s\": bad PNG filter type %d", filename, (int) filter);
            }
            row[x] = (unsigned char) v;
        }
    }
    const float *table = srgbTable();
    rgb.resize((size_t) width * height * 3);
    for (size_t p = 0; p < (size_t) width * height; ++p)
        for (int k = 0; k < 3; ++k) {
            const unsigned char v = px[p * channels + (channels >= 3 ? k : 0)];
            rgb[3 * p + k] = srgb ? table[v] : (float) (v / 255.0);
        }
}

bool hasExtension(const std::string &s, const std::string &suffix) {
    if (s.size() < suffix.size()) return false;
    std::string tail = s.substr(s.size() - suffix.size());
    for (char &ch : tail) ch = (char) std::tolower((unsigned char) ch);
    return tail == suffix;
}

/* filter, wrap, scale and offset: common to both textures */
struct Mapping {
    int filter = NORI_FILTER_BILINEAR, wrap = NORI_WRAP_REPEAT;
    float uscale = 1.0f, vscale = 1.0f, uoffset = 0.0f, voffset = 0.0f;
    explicit Mapping(const PropertyList &p) {
        const std::string f = p.getString("filter", "bilinear"), w = p.getString("wrap", "repeat");
        if (f == "nearest") filter = NORI_FILTER_NEAREST;
        else if (f != "bilinear") throw NoriException("texture: unknown filter \"%s\" (bilinear or nearest)", f);
        if (w == "clamp") wrap = NORI_WRAP_CLAMP;
        else if (w != "repeat") throw NoriException("texture: unknown wrap mode \"%s\" (repeat or clamp)", w);
        uscale = p.getFloat("uscale", 1.0f); vscale = p.getFloat("vscale", 1.0f);
        uoffset = p.getFloat("uoffset", 0.0f); voffset = p.getFloat("voffset", 0.0f);
    }
    void fill(nori_texture_desc &d) const {
        d.filter = filter; d.wrap = wrap; d.uscale = uscale; d.vscale = vscale; d.uoffset = uoffset; d.voffset = voffset;
    }
};

} // namespace

class ImageTexture : public Texture {
public:
    ImageTexture(const PropertyList &propList) : m_map(propList) {
        m_filename = getFileResolver()->resolve(propList.getString("filename"));
        const bool exr = hasExtension(m_filename, ".exr"), png = hasExtension(m_filename, ".png");
        if (!exr && !png) throw NoriException("texture: unsupported image \"%s\" (PNG or OpenEXR)", m_filename);
        const bool srgb = propList.getBoolean("srgb", png);
        if (png) {
            loadPNG(m_filename, srgb, m_width, m_height, m_texels);
        } else {
            {
                std::ifstream probe(m_filename, std::ios::binary);
                if (probe.fail()) throw NoriException("cannot read image \"%s\"", m_filename);
            }
            Bitmap b(m_filename);
            if (b.cols() <= 0 || b.rows() <= 0 || b.cols() > 16384 || b.rows() > 16384)
                throw NoriException("\"%s\": image of %d x %d pixels (each dimension must be 1 .. 16384)", m_filename, b.cols(), b.rows());
            m_width = (uint32_t) b.cols(); m_height = (uint32_t) b.rows();
            m_texels.assign(b.data(), b.data() + (size_t) m_width * m_height * 3);
            if (srgb) for (float &v : m_texels) v = (float) srgbToLinear((double) v);
        }
    }
    void fill(nori_texture_desc &d) const {
        std::memset(&d, 0, sizeof(d));
        d.type = NORI_TEXTURE_IMAGE;
        d.width = m_width; d.height = m_height; d.texels = m_texels.data();
        m_map.fill(d);
    }
    std::string toString() const { return format("ImageTexture[\n  filename = \"%s\",\n  size = %u x %u\n]", m_filename, m_width, m_height); }
private:
    Mapping m_map;
    std::string m_filename;
    uint32_t m_width = 0, m_height = 0;
    std::vector<float> m_texels;
};

class CheckerboardTexture : public Texture {
public:
    CheckerboardTexture(const PropertyList &propList) : m_map(propList) {
        m_color0 = propList.getColor("color0", Color3f(0.4f));
        m_color1 = propList.getColor("color1", Color3f(0.2f));
    }
    void fill(nori_texture_desc &d) const {
        std::memset(&d, 0, sizeof(d));
        d.type = NORI_TEXTURE_CHECKERBOARD;
        m_map.fill(d);
        for (int k = 0; k < 3; ++k) { d.color0[k] = m_color0[k]; d.color1[k] = m_color1[k]; }
    }
    std::string toString() const { return format("CheckerboardTexture[\n  color0 = %s,\n  color1 = %s\n]", m_color0.toString(), m_color1.toString()); }
private:
    Mapping m_map;
    Color3f m_color0, m_color1;
};

NORI_REGISTER_CLASS(ImageTexture, "image");
NORI_REGISTER_CLASS(CheckerboardTexture, "checkerboard");

NORI_NAMESPACE_END
