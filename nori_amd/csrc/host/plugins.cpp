/*
 * plugins.cpp -- host side of the plugin surface.
 *
 * Registered names (what the XML `type=` attribute selects), with the
 * reference's parameter names and defaults:
 *   bsdf        diffuse (src/diffuse.cpp:18-20), mirror (src/mirror.cpp:15),
 *               dielectric (src/dielectric.cpp:17-23), microfacet (src/microfacet.cpp:17-36)
 *   emitter     area  [radiance]                          (absent from the reference)
 *   integrator  normals, ao, simple [position, energy], whitted, path_mats,
 *               path_ems, path_mis                        (absent from the reference)
 *   sampler     independent [sampleCount]                 (src/independent.cpp:23-25)
 *   camera      perspective                               (src/perspective.cpp:22-39)
 *   rfilter     gaussian, mitchell, tent, box             (src/rfilter.cpp)
 * None of these classes computes radiance, samples or intersections on the
 * CPU: the virtuals forward to libnori_hip.
 */
#include <nori/plugins.h>
#include <nori/bitmap.h>

#include <algorithm>
#include <cmath>
#include <cstring>
#include <fstream>

NORI_NAMESPACE_BEGIN

/* =================================================================== Warp */
void Warp::warpBatch(nori_warp_type type, float param, const float *samples, size_t n, float *out) {
    Device &d = Device::shared();
    d.check(nori_hip_warp(d.ctx(), type, param, samples, n, out), "nori_hip_warp");
}
void Warp::pdfBatch(nori_warp_type type, float param, const float *points, size_t n, float *pdf) {
    Device &d = Device::shared();
    d.check(nori_hip_warp_pdf(d.ctx(), type, param, points, n, pdf), "nori_hip_warp_pdf");
}
static Vector3f warp1(nori_warp_type t, float param, const Point2f &s) {
    float in[2] = {s.x(), s.y()}, out[3];
    Warp::warpBatch(t, param, in, 1, out);
    return Vector3f(out[0], out[1], out[2]);
}
static float pdf1(nori_warp_type t, float param, const Vector3f &v) {
    float in[3] = {v.x(), v.y(), v.z()}, out;
    Warp::pdfBatch(t, param, in, 1, &out);
    return out;
}
Point2f Warp::squareToUniformSquare(const Point2f &s) { Vector3f r = warp1(NORI_WARP_SQUARE, 0, s); return Point2f(r.x(), r.y()); }
float Warp::squareToUniformSquarePdf(const Point2f &p) { return pdf1(NORI_WARP_SQUARE, 0, Vector3f(p.x(), p.y(), 0)); }
Point2f Warp::squareToTent(const Point2f &s) { Vector3f r = warp1(NORI_WARP_TENT, 0, s); return Point2f(r.x(), r.y()); }
float Warp::squareToTentPdf(const Point2f &p) { return pdf1(NORI_WARP_TENT, 0, Vector3f(p.x(), p.y(), 0)); }
Point2f Warp::squareToUniformDisk(const Point2f &s) { Vector3f r = warp1(NORI_WARP_DISK, 0, s); return Point2f(r.x(), r.y()); }
float Warp::squareToUniformDiskPdf(const Point2f &p) { return pdf1(NORI_WARP_DISK, 0, Vector3f(p.x(), p.y(), 0)); }
Vector3f Warp::squareToUniformSphere(const Point2f &s) { return warp1(NORI_WARP_UNIFORM_SPHERE, 0, s); }
float Warp::squareToUniformSpherePdf(const Vector3f &v) { return pdf1(NORI_WARP_UNIFORM_SPHERE, 0, v); }
Vector3f Warp::squareToUniformHemisphere(const Point2f &s) { return warp1(NORI_WARP_UNIFORM_HEMISPHERE, 0, s); }
float Warp::squareToUniformHemispherePdf(const Vector3f &v) { return pdf1(NORI_WARP_UNIFORM_HEMISPHERE, 0, v); }
Vector3f Warp::squareToCosineHemisphere(const Point2f &s) { return warp1(NORI_WARP_COSINE_HEMISPHERE, 0, s); }
float Warp::squareToCosineHemispherePdf(const Vector3f &v) { return pdf1(NORI_WARP_COSINE_HEMISPHERE, 0, v); }
Vector3f Warp::squareToBeckmann(const Point2f &s, float alpha) { return warp1(NORI_WARP_BECKMANN, alpha, s); }
float Warp::squareToBeckmannPdf(const Vector3f &m, float alpha) { return pdf1(NORI_WARP_BECKMANN, alpha, m); }

/* =================================================================== BSDF */
void BSDF::sampleBatch(const float *wi, const float *sample, size_t n, float *wo, float *weight, float *eta, int32_t *measure) const {
    nori_bsdf_desc d; fill(d);
    Device &dev = Device::shared();
    dev.check(nori_hip_bsdf_sample(dev.ctx(), &d, wi, sample, n, wo, weight, eta, measure), "nori_hip_bsdf_sample");
}
void BSDF::evalBatch(const float *wi, const float *wo, size_t n, float *value) const {
    nori_bsdf_desc d; fill(d);
    Device &dev = Device::shared();
    dev.check(nori_hip_bsdf_eval(dev.ctx(), &d, wi, wo, n, value), "nori_hip_bsdf_eval");
}
void BSDF::pdfBatch(const float *wi, const float *wo, size_t n, float *pdf) const {
    nori_bsdf_desc d; fill(d);
    Device &dev = Device::shared();
    dev.check(nori_hip_bsdf_pdf(dev.ctx(), &d, wi, wo, n, pdf), "nori_hip_bsdf_pdf");
}
Color3f BSDF::sample(BSDFQueryRecord &bRec, const Point2f &s) const {
    float wo[3], w[3], eta; int32_t m;
    sampleBatch(bRec.wi.v, s.v, 1, wo, w, &eta, &m);
    bRec.wo = Vector3f(wo[0], wo[1], wo[2]); bRec.eta = eta; bRec.measure = (EMeasure) m;
    return Color3f(w[0], w[1], w[2]);
}
Color3f BSDF::eval(const BSDFQueryRecord &bRec) const {
    if (bRec.measure != ESolidAngle) return Color3f(0.0f);       /* src/diffuse.cpp:26 */
    float v[3];
    evalBatch(bRec.wi.v, bRec.wo.v, 1, v);
    return Color3f(v[0], v[1], v[2]);
}
float BSDF::pdf(const BSDFQueryRecord &bRec) const {
    if (bRec.measure != ESolidAngle) return 0.0f;
    float p;
    pdfBatch(bRec.wi.v, bRec.wo.v, 1, &p);
    return p;
}

static void clearDesc(nori_bsdf_desc &d, int type) { std::memset(&d, 0, sizeof(d)); d.type = type; }

void BSDF::addChild(NoriObject *child) {
    if (child->getClassType() == ETexture) {
        const std::string s = toString();
        throw NoriException("a <texture> can only be the albedo of a diffuse BSDF, not of %s", s.substr(0, s.find('[')));
    }
    NoriObject::addChild(child);
}

class Diffuse : public BSDF {
public:
    Diffuse(const PropertyList &propList) {
        m_albedo = propList.getColor("albedo", Color3f(0.5f));
        m_hasAlbedo = propList.has("albedo");
    }
    ~Diffuse() { delete m_texture; }
    bool isDiffuse() const { return true; }
    /* <texture name="albedo"> in place of <color name="albedo"> */
    void addChild(NoriObject *child) {
        if (child->getClassType() != ETexture) { BSDF::addChild(child); return; }
        if (m_hasAlbedo) throw NoriException("a diffuse BSDF cannot have both an albedo color and an albedo texture");
        if (m_texture) throw NoriException("a diffuse BSDF can only have one albedo texture");
        m_texture = static_cast<Texture *>(child);
    }
    const Texture *albedoTexture() const { return m_texture; }
    void fill(nori_bsdf_desc &d) const { clearDesc(d, NORI_BSDF_DIFFUSE); for (int i = 0; i < 3; ++i) d.albedo[i] = m_albedo[i]; }
    std::string toString() const { return format("Diffuse[\n  albedo = %s\n]", m_texture ? indent(m_texture->toString()) : m_albedo.toString()); }
private:
    Color3f m_albedo;
    bool m_hasAlbedo = false;
    Texture *m_texture = nullptr;
};

class Mirror : public BSDF {
public:
    Mirror(const PropertyList &) {}
    void fill(nori_bsdf_desc &d) const { clearDesc(d, NORI_BSDF_MIRROR); }
    std::string toString() const { return "Mirror[]"; }
};

class Dielectric : public BSDF {
public:
    Dielectric(const PropertyList &propList) {
        m_intIOR = propList.getFloat("intIOR", 1.5046f);     /* BK7 */
        m_extIOR = propList.getFloat("extIOR", 1.000277f);   /* air */
    }
    void fill(nori_bsdf_desc &d) const { clearDesc(d, NORI_BSDF_DIELECTRIC); d.int_ior = m_intIOR; d.ext_ior = m_extIOR; }
    std::string toString() const { return format("Dielectric[\n  intIOR = %f,\n  extIOR = %f\n]", m_intIOR, m_extIOR); }
private:
    float m_intIOR, m_extIOR;
};

class Microfacet : public BSDF {
public:
    Microfacet(const PropertyList &propList) {
        m_alpha = propList.getFloat("alpha", 0.1f);
        m_intIOR = propList.getFloat("intIOR", 1.5046f);
        m_extIOR = propList.getFloat("extIOR", 1.000277f);
        m_kd = propList.getColor("kd", Color3f(0.5f));
        m_ks = 1 - m_kd.maxCoeff();                           /* src/microfacet.cpp:35 */
    }
    bool isDiffuse() const { return true; }                   /* src/microfacet.cpp:59-64 */
    void fill(nori_bsdf_desc &d) const {
        clearDesc(d, NORI_BSDF_MICROFACET);
        for (int i = 0; i < 3; ++i) d.albedo[i] = m_kd[i];
        d.alpha = m_alpha; d.int_ior = m_intIOR; d.ext_ior = m_extIOR; d.ks = m_ks;
    }
    std::string toString() const {
        return format("Microfacet[\n  alpha = %f,\n  intIOR = %f,\n  extIOR = %f,\n  kd = %s,\n  ks = %f\n]",
                      m_alpha, m_intIOR, m_extIOR, m_kd.toString(), m_ks);
    }
private:
    float m_alpha, m_intIOR, m_extIOR, m_ks;
    Color3f m_kd;
};

NORI_REGISTER_CLASS(Diffuse, "diffuse");
NORI_REGISTER_CLASS(Mirror, "mirror");
NORI_REGISTER_CLASS(Dielectric, "dielectric");
NORI_REGISTER_CLASS(Microfacet, "microfacet");

/* ================================================================ Emitter */
class AreaLight : public Emitter {
public:
    AreaLight(const PropertyList &propList) { m_radiance = propList.getColor("radiance"); }
    Color3f getRadiance() const { return m_radiance; }
    std::string toString() const { return format("AreaLight[\n  radiance = %s\n]", m_radiance.toString()); }
private:
    Color3f m_radiance;
};
NORI_REGISTER_CLASS(AreaLight, "area");

/* <emitter type="envmap"> as a child of <scene>: image-based lighting (include/nori_hip.h, "Environment-map emitter").
 *   filename    a latitude-longitude OpenEXR image, y up: a local direction (x, y, z) is looked up at phi = atan2(x, -z) across
 *               (the image's middle column looks down -z), theta = acos(y) down (row 0 is +y)
 *   scale       colour, multiplies the map (default 1)
 *   resolution  N of the octahedral map the device samples (default 512, 1 .. 4096)
 *   toWorld     its rotation part turns the map (world = M local); anything else in it is ignored
 * The device's map is octahedral, so the image is resampled here, once: at the centre of each of the N x N texels the direction is
 * taken back to (phi, theta) and the image is read bilinearly (wrapping across, clamped at the poles), in double precision with
 * the host's libm.  This is a choice of texel values, outside the path the parity claims cover: what the device does with the
 * texels it is given is what the header pins. */
class EnvironmentMap : public Emitter {
public:
    EnvironmentMap(const PropertyList &propList) {
        m_filename = getFileResolver()->resolve(propList.getString("filename"));
        if (m_filename.size() < 4 || toLower(m_filename.substr(m_filename.size() - 4)) != ".exr") throw NoriException("envmap: unsupported image \"%s\" (a latitude-longitude OpenEXR file)", m_filename);
        m_scale = propList.getColor("scale", Color3f(1.0f));
        for (int c = 0; c < 3; ++c)
            if (!std::isfinite(m_scale[c]) || m_scale[c] < 0.0f) throw NoriException("envmap: scale must be finite and not negative");
        const int res = propList.getInteger("resolution", 512);
        if (res < 1 || res > 4096) throw NoriException("envmap: resolution must be 1 .. 4096 (got %d)", res);
        m_size = (uint32_t) res;
        const Transform t = propList.getTransform("toWorld", Transform());
        for (int r = 0; r < 3; ++r) for (int c = 0; c < 3; ++c) m_toWorld[3 * r + c] = t.m[4 * r + c];
        for (int a = 0; a < 3; ++a)
            for (int b = a; b < 3; ++b) {
                double d = 0.0;
                for (int k = 0; k < 3; ++k) d += (double) m_toWorld[3 * a + k] * m_toWorld[3 * b + k];
                if (!(std::fabs(d - (a == b ? 1.0 : 0.0)) <= 1e-4)) throw NoriException("envmap: toWorld must be a rotation (its upper 3 x 3 rows are not orthonormal)");
            }
        {
            std::ifstream probe(m_filename, std::ios::binary);
            if (probe.fail()) throw NoriException("cannot read image \"%s\"", m_filename);
        }
        Bitmap img(m_filename);
        if (img.cols() <= 0 || img.rows() <= 0) throw NoriException("\"%s\": empty image", m_filename);
        resample(img);
    }
    Color3f getRadiance() const { return Color3f(0.0f); }
    bool isEnvironment() const { return true; }
    void fillEnvironment(nori_env_desc &d) const {
        std::memset(&d, 0, sizeof(d));
        d.size = m_size; d.texels = m_texels.data();
        for (int c = 0; c < 3; ++c) d.scale[c] = m_scale[c];
        for (int k = 0; k < 9; ++k) d.to_world[k] = m_toWorld[k];
    }
    std::string toString() const { return format("EnvironmentMap[\n  filename = \"%s\",\n  resolution = %u,\n  scale = %s\n]", m_filename, m_size, m_scale.toString()); }
private:
    void resample(const Bitmap &img) {
        const int W = img.cols(), H = img.rows(), N = (int) m_size;
        m_texels.resize((size_t) N * N * 3);
        double sum = 0.0;
        for (int j = 0; j < N; ++j)
            for (int i = 0; i < N; ++i) {
                /* the texel centre's direction: the inverse of the header's "Direction -> texel" */
                double px = 2.0 * ((i + 0.5) / N) - 1.0, py = 2.0 * ((j + 0.5) / N) - 1.0;
                const double pz = 1.0 - std::fabs(px) - std::fabs(py);
                if (pz < 0.0) {
                    const double ox = px, oy = py;
                    px = (1.0 - std::fabs(oy)) * (ox >= 0.0 ? 1.0 : -1.0);
                    py = (1.0 - std::fabs(ox)) * (oy >= 0.0 ? 1.0 : -1.0);
                }
                const double len = std::sqrt(px * px + py * py + pz * pz);
                const double x = px / len, y = py / len, z = pz / len;
                const double phi = std::atan2(x, -z), theta = std::acos(std::min(1.0, std::max(-1.0, y)));
                const double fx = (phi / (2.0 * M_PI) + 0.5) * W - 0.5, fy = theta / M_PI * H - 0.5;
                const double x0 = std::floor(fx), y0 = std::floor(fy), ax = fx - x0, ay = fy - y0;
                auto col = [W](int c) { c %= W; return c < 0 ? c + W : c; };
                auto row = [H](int r) { return r < 0 ? 0 : (r > H - 1 ? H - 1 : r); };
                const int c0 = col((int) x0), c1 = col((int) x0 + 1), r0 = row((int) y0), r1 = row((int) y0 + 1);
                for (int c = 0; c < 3; ++c) {
                    const double top = (1.0 - ax) * img.coeff(r0, c0)[c] + ax * img.coeff(r0, c1)[c];
                    const double bot = (1.0 - ax) * img.coeff(r1, c0)[c] + ax * img.coeff(r1, c1)[c];
                    const float v = (float) ((1.0 - ay) * top + ay * bot);
                    if (!std::isfinite(v) || v < 0.0f) throw NoriException("\"%s\": a pixel is negative or not finite", m_filename);
                    m_texels[((size_t) j * N + i) * 3 + c] = v;
                    sum += (double) v * m_scale[c];
                }
            }
        if (!(sum > 0.0)) throw NoriException("envmap: \"%s\" times scale is black everywhere (nothing to light the scene with)", m_filename);
    }
    std::string m_filename;
    Color3f m_scale;
    uint32_t m_size = 0;
    float m_toWorld[9];
    std::vector<float> m_texels;
};
NORI_REGISTER_CLASS(EnvironmentMap, "envmap");

/* <emitter type="point|spot|directional"> as children of <scene>: delta lights (include/nori_hip.h, "Delta lights").
 *   point        position (point); intensity (color, W/sr) or power (color, W): I = power (kInvPi 0.25f)
 *   spot         position (point); direction (vector) or target (point: direction = target - position); intensity (color);
 *                cutoffAngle (degrees from the axis where the light ends, default 20) and beamWidth (degrees within which it is
 *                full, default 3/4 of cutoffAngle): cos_outer = cos(cutoffAngle), cos_inner = cos(beamWidth)
 *   directional  direction (vector, the way the light travels); irradiance (color)
 * What nori_hip_set_lights would refuse of one light is said here, before a device is asked for. */
class DeltaLight : public Emitter {
public:
    DeltaLight(const PropertyList &propList, int type, const char *name) {
        std::memset(&m_desc, 0, sizeof(m_desc));
        m_desc.type = type;
        if (type != NORI_LIGHT_DIRECTIONAL) {
            const Point3f p = propList.getPoint("position");
            for (int c = 0; c < 3; ++c) m_desc.position[c] = p[c];
        }
        Color3f I;
        if (type == NORI_LIGHT_DIRECTIONAL) I = propList.getColor("irradiance");
        else if (propList.has("power")) {
            if (propList.has("intensity")) throw NoriException("%s light: give intensity or power, not both", name);
            if (type == NORI_LIGHT_SPOT) throw NoriException("spot light: give its intensity (its power depends on the cone)");
            I = propList.getColor("power") * (0.31830988618379067154f * 0.25f);
        } else I = propList.getColor("intensity");
        for (int c = 0; c < 3; ++c) {
            if (!std::isfinite(I[c]) || I[c] < 0.0f) throw NoriException("%s light: every component of %s must be finite and not negative", name, type == NORI_LIGHT_DIRECTIONAL ? "irradiance" : "intensity");
            if (!std::isfinite(m_desc.position[c])) throw NoriException("%s light: position must be finite", name);
            m_desc.intensity[c] = I[c];
        }
        if (type != NORI_LIGHT_POINT) {
            Vector3f d;
            if (type == NORI_LIGHT_SPOT && propList.has("target")) {
                if (propList.has("direction")) throw NoriException("spot light: give direction or target, not both");
                const Point3f t = propList.getPoint("target");
                d = Vector3f(t[0] - m_desc.position[0], t[1] - m_desc.position[1], t[2] - m_desc.position[2]);
            } else d = propList.getVector("direction");
            const float z = d[0] * d[0] + (d[1] * d[1] + d[2] * d[2]);
            if (!(z > 0.0f) || !std::isfinite(z)) throw NoriException("%s light: direction must be finite and of non-zero length", name);
            for (int c = 0; c < 3; ++c) m_desc.direction[c] = d[c];
        }
        if (type == NORI_LIGHT_SPOT) {
            const float cutoff = propList.getFloat("cutoffAngle", 20.0f), beam = propList.getFloat("beamWidth", cutoff * 0.75f);
            if (!(cutoff > 0.0f && cutoff <= 180.0f)) throw NoriException("spot light: cutoffAngle must lie in (0, 180] degrees (got %f)", cutoff);
            if (!(beam >= 0.0f && beam <= cutoff)) throw NoriException("spot light: beamWidth must lie in [0, cutoffAngle] degrees (got %f)", beam);
            m_desc.cos_outer = (float) std::cos((double) cutoff * M_PI / 180.0);
            m_desc.cos_inner = (float) std::cos((double) beam * M_PI / 180.0);
        }
    }
    Color3f getRadiance() const { return Color3f(0.0f); }
    bool isDeltaLight() const { return true; }
    void fillLight(nori_light_desc &d) const { d = m_desc; }
    std::string toString() const {
        return format("DeltaLight[\n  type = %d,\n  intensity = [%f, %f, %f]\n]", m_desc.type, m_desc.intensity[0], m_desc.intensity[1], m_desc.intensity[2]);
    }
private:
    nori_light_desc m_desc;
};
class PointLight : public DeltaLight { public: PointLight(const PropertyList &p) : DeltaLight(p, NORI_LIGHT_POINT, "point") {} };
class SpotLight : public DeltaLight { public: SpotLight(const PropertyList &p) : DeltaLight(p, NORI_LIGHT_SPOT, "spot") {} };
class DirectionalLight : public DeltaLight { public: DirectionalLight(const PropertyList &p) : DeltaLight(p, NORI_LIGHT_DIRECTIONAL, "directional") {} };
NORI_REGISTER_CLASS(PointLight, "point");
NORI_REGISTER_CLASS(SpotLight, "spot");
NORI_REGISTER_CLASS(DirectionalLight, "directional");

/* ================================================= Medium, PhaseFunction */
/* <phase type="isotropic"/> */
class IsotropicPhase : public PhaseFunction {
public:
    IsotropicPhase(const PropertyList &) {}
    float getAsymmetry() const { return 0.0f; }
    std::string toString() const { return "Isotropic[]"; }
};
NORI_REGISTER_CLASS(IsotropicPhase, "isotropic");

/* <phase type="hg"><float name="g" value="..."/></phase>: Henyey-Greenstein, g > 0 scatters forward; |g| <= 0.99 */
class HenyeyGreensteinPhase : public PhaseFunction {
public:
    HenyeyGreensteinPhase(const PropertyList &propList) {
        m_g = propList.getFloat("g", 0.0f);
        if (!(std::fabs(m_g) <= 0.99f)) throw NoriException("phase hg: g must lie in [-0.99, 0.99] (got %f)", m_g);
    }
    float getAsymmetry() const { return m_g; }
    std::string toString() const { return format("HenyeyGreenstein[g = %f]", m_g); }
private:
    float m_g;
};
NORI_REGISTER_CLASS(HenyeyGreensteinPhase, "hg");

/* <medium type="homogeneous"> as a child of <scene> (include/nori_hip.h, "Homogeneous participating medium"): it fills all space.
 *   sigmaT    float, the grey extinction, 1e-4 .. 1e4
 *   albedo    color, the single-scattering albedo, each component 0 .. 1 (default 1)
 *   <phase>   an optional child: isotropic (the default) or hg */
class HomogeneousMedium : public Medium {
public:
    HomogeneousMedium(const PropertyList &propList) {
        m_sigmaT = propList.getFloat("sigmaT");
        if (!(std::isfinite(m_sigmaT) && m_sigmaT >= 1e-4f && m_sigmaT <= 1e4f)) throw NoriException("medium: sigmaT must lie in [1e-4, 1e4] (got %f)", m_sigmaT);
        m_albedo = propList.getColor("albedo", Color3f(1.0f));
        for (int c = 0; c < 3; ++c)
            if (!(std::isfinite(m_albedo[c]) && m_albedo[c] >= 0.0f && m_albedo[c] <= 1.0f)) throw NoriException("medium: every albedo component must lie in [0, 1]");
    }
    ~HomogeneousMedium() { delete m_phase; }
    void addChild(NoriObject *obj) {
        if (obj->getClassType() != EPhaseFunction) throw NoriException("Medium::addChild(<%s>) is not supported!", classTypeName(obj->getClassType()));
        if (m_phase) throw NoriException("There can only be one phase function per medium!");
        m_phase = static_cast<PhaseFunction *>(obj);
    }
    void fillMedium(nori_medium_desc &d) const {
        d.sigma_t = m_sigmaT;
        for (int c = 0; c < 3; ++c) d.albedo[c] = m_albedo[c];
        d.g = m_phase ? m_phase->getAsymmetry() : 0.0f;
    }
    std::string toString() const {
        return format("HomogeneousMedium[\n  sigmaT = %f,\n  albedo = %s,\n  phase = %s\n]", m_sigmaT, m_albedo.toString(),
                      m_phase ? indent(m_phase->toString()) : std::string("Isotropic[]"));
    }
private:
    float m_sigmaT;
    Color3f m_albedo;
    PhaseFunction *m_phase = nullptr;
};
NORI_REGISTER_CLASS(HomogeneousMedium, "homogeneous");

/* <medium type="grid"> as a child of <scene> (include/nori_hip.h, "Grid medium"): a box of voxels of piecewise-constant density.
 *   filename     string, a VOL file, little-endian: the bytes 'V' 'O' 'L', a version byte 3, int32 encoding 1 (float32), int32 nx, ny, nz,
 *                int32 channels 1, six float32 xmin ymin zmin xmax ymax zmax, then nx ny nz float32 with x fastest
 *   sigmaScale   float, a voxel's extinction is sigmaScale rho: 0, or 1e-4 .. 1e4 (default 1)
 *   albedo       color, the single-scattering albedo, each component 0 .. 1 (default 1)
 *   boxMin, boxMax   points, optional: they override the file's box
 *   <phase>      an optional child: isotropic (the default) or hg
 * What nori_hip_set_grid_medium would refuse of the grid is said here, before a device is asked for. */
class GridMedium : public Medium {
public:
    GridMedium(const PropertyList &propList) {
        m_filename = getFileResolver()->resolve(propList.getString("filename"));
        std::ifstream is(m_filename, std::ios::binary);
        if (!is) throw NoriException("medium grid: cannot open \"%s\"", m_filename);
        char magic[4] = {0, 0, 0, 0};
        int32_t head[5] = {0, 0, 0, 0, 0};
        float box[6];
        is.read(magic, 4);
        is.read(reinterpret_cast<char *>(head), sizeof(head));
        is.read(reinterpret_cast<char *>(box), sizeof(box));
        if (!is || magic[0] != 'V' || magic[1] != 'O' || magic[2] != 'L' || magic[3] != 3)
            throw NoriException("medium grid: \"%s\" is not a VOL file of version 3", m_filename);
        if (head[0] != 1) throw NoriException("medium grid: \"%s\": encoding %d, only 1 (float32) is read", m_filename, head[0]);
        if (head[4] != 1) throw NoriException("medium grid: \"%s\": %d channels, only 1 is read", m_filename, head[4]);
        for (int a = 0; a < 3; ++a) {
            m_n[a] = head[1 + a];
            if (m_n[a] < 1 || m_n[a] > 256) throw NoriException("medium grid: nx, ny and nz must each lie in 1 .. 256 (got %d x %d x %d)", head[1], head[2], head[3]);
            m_bmin[a] = box[a]; m_bmax[a] = box[3 + a];
        }
        if (propList.has("boxMin")) { const Point3f p = propList.getPoint("boxMin"); for (int a = 0; a < 3; ++a) m_bmin[a] = p[a]; }
        if (propList.has("boxMax")) { const Point3f p = propList.getPoint("boxMax"); for (int a = 0; a < 3; ++a) m_bmax[a] = p[a]; }
        for (int a = 0; a < 3; ++a)
            if (!(std::isfinite(m_bmin[a]) && std::isfinite(m_bmax[a]) && m_bmin[a] < m_bmax[a] && std::isfinite(m_bmax[a] - m_bmin[a])))
                throw NoriException("medium grid: the box needs finite boxMin < boxMax on every axis (axis %d: %f, %f)", a, m_bmin[a], m_bmax[a]);
        m_sigmaScale = propList.getFloat("sigmaScale", 1.0f);
        if (!std::isfinite(m_sigmaScale) || !(m_sigmaScale >= 0.0f)) throw NoriException("medium grid: sigmaScale must be finite and not negative (got %f)", m_sigmaScale);
        m_albedo = propList.getColor("albedo", Color3f(1.0f));
        for (int c = 0; c < 3; ++c)
            if (!(std::isfinite(m_albedo[c]) && m_albedo[c] >= 0.0f && m_albedo[c] <= 1.0f)) throw NoriException("medium: every albedo component must lie in [0, 1]");
        const size_t n = (size_t) m_n[0] * (size_t) m_n[1] * (size_t) m_n[2];
        m_rho.resize(n);
        is.read(reinterpret_cast<char *>(m_rho.data()), (std::streamsize) (n * sizeof(float)));
        if (!is) throw NoriException("medium grid: \"%s\" ends before its %d x %d x %d voxels", m_filename, m_n[0], m_n[1], m_n[2]);
        for (size_t k = 0; k < n; ++k) {
            const float rho = m_rho[k], sigma = m_sigmaScale * rho;
            if (!(std::isfinite(rho) && rho >= 0.0f && (sigma == 0.0f || (sigma >= 1e-4f && sigma <= 1e4f))))
                throw NoriException("medium grid: voxel %d: rho must be finite and not negative, and sigmaScale * rho 0 or in [1e-4, 1e4] (rho %f)", (int) k, rho);
        }
    }
    ~GridMedium() { delete m_phase; }
    void addChild(NoriObject *obj) {
        if (obj->getClassType() != EPhaseFunction) throw NoriException("Medium::addChild(<%s>) is not supported!", classTypeName(obj->getClassType()));
        if (m_phase) throw NoriException("There can only be one phase function per medium!");
        m_phase = static_cast<PhaseFunction *>(obj);
    }
    void fillMedium(nori_medium_desc &d) const { std::memset(&d, 0, sizeof(d)); }
    bool isGrid() const { return true; }
    void fillGridMedium(nori_grid_medium_desc &d) const {
        d.rho = m_rho.data();
        d.nx = m_n[0]; d.ny = m_n[1]; d.nz = m_n[2];
        for (int a = 0; a < 3; ++a) { d.bmin[a] = m_bmin[a]; d.bmax[a] = m_bmax[a]; d.albedo[a] = m_albedo[a]; }
        d.sigma_scale = m_sigmaScale;
        d.g = m_phase ? m_phase->getAsymmetry() : 0.0f;
    }
    std::string toString() const {
        return format("GridMedium[\n  filename = \"%s\",\n  voxels = %d x %d x %d,\n  sigmaScale = %f,\n  albedo = %s,\n  phase = %s\n]", m_filename, m_n[0], m_n[1], m_n[2],
                      m_sigmaScale, m_albedo.toString(), m_phase ? indent(m_phase->toString()) : std::string("Isotropic[]"));
    }
private:
    std::string m_filename;
    int32_t m_n[3];
    float m_bmin[3], m_bmax[3], m_sigmaScale;
    Color3f m_albedo;
    std::vector<float> m_rho;
    PhaseFunction *m_phase = nullptr;
};
NORI_REGISTER_CLASS(GridMedium, "grid");

/* ================================================================ Sampler */
/* src/independent.cpp:21-67.  The pcg32 arithmetic runs on the device
   (nori_hip_pcg32_floats_at); the host keeps the stream key, how many numbers of the stream it has
   handed out, and a buffer.  prepare(block) = m_random.seed(offset.x, offset.y)
   (independent.cpp:36-41): next1D / next2D then walk exactly the reference's pcg32 sequence, however the
   buffer is refilled and whatever blocks were rendered before. */
class Independent : public Sampler {
public:
    Independent(const PropertyList &propList) { m_sampleCount = (size_t) propList.getInteger("sampleCount", 1); }
    std::unique_ptr<Sampler> clone() const {
        std::unique_ptr<Independent> c(new Independent());
        /* the reference copies m_random, i.e. the position in the stream too (independent.cpp:30-34) */
        c->m_sampleCount = m_sampleCount; c->m_state = m_state; c->m_seq = m_seq; c->m_forks = m_forks;
        c->m_drawn = m_drawn - (m_buffer.size() - m_pos);
        return std::move(c);
    }
    void prepare(const ImageBlock &block) {
        m_state = (uint64_t) block.getOffset().x(); m_seq = (uint64_t) block.getOffset().y();
        m_buffer.clear(); m_pos = 0; m_forks = 0; m_drawn = 0;
    }
    void generate() {}
    void advance() {}
    float next1D() {
        if (m_pos >= m_buffer.size()) refill();
        return m_buffer[m_pos++];
    }
    Point2f next2D() { float a = next1D(); float b = next1D(); return Point2f(a, b); }
    void forkStream(uint64_t &state, uint64_t &seq) {
        /* distinct pcg32 streams per path: same initstate, initseq advanced in a
           range disjoint from the refill streams */
        state = m_state; seq = (m_seq << 32) + 0x80000000ull + m_forks++;      /* never equal to the block's own initseq (< 2^31) */
    }
    std::string toString() const { return format("Independent[sampleCount=%i]", (int) m_sampleCount); }
protected:
    Independent() {}
private:
    void refill() {
        const uint32_t kChunk = 4096;
        m_buffer.resize(kChunk);
        uint64_t st = m_state, sq = m_seq;
        Device &d = Device::shared();
        d.check(nori_hip_pcg32_floats_at(d.ctx(), &st, &sq, m_drawn, 1, kChunk, m_buffer.data()), "nori_hip_pcg32_floats_at");
        m_drawn += kChunk;        /* numbers of the stream fetched so far */
        m_pos = 0;
    }
    uint64_t m_state = 0x853c49e6748fea9bULL, m_seq = 0xda3e39cb94b95bdbULL >> 1, m_forks = 0, m_drawn = 0;
    std::vector<float> m_buffer;
    size_t m_pos = 0;
};
NORI_REGISTER_CLASS(Independent, "independent");

/* ================================================================ Filters */
class GaussianFilter : public ReconstructionFilter {
public:
    GaussianFilter(const PropertyList &propList) {
        m_radius = propList.getFloat("radius", 2.0f);
        m_stddev = propList.getFloat("stddev", 0.5f);
    }
    float eval(float x) const {
        float alpha = -1.0f / (2.0f * m_stddev * m_stddev);
        return std::max(0.0f, std::exp(alpha * x * x) - std::exp(alpha * m_radius * m_radius));
    }
    void fill(nori_rfilter_desc &d) const { std::memset(&d, 0, sizeof(d)); d.type = NORI_RFILTER_GAUSSIAN; d.radius = m_radius; d.stddev = m_stddev; }
    std::string toString() const { return format("GaussianFilter[radius=%f, stddev=%f]", m_radius, m_stddev); }
protected:
    float m_stddev;
};

class MitchellNetravaliFilter : public ReconstructionFilter {
public:
    MitchellNetravaliFilter(const PropertyList &propList) {
        m_radius = propList.getFloat("radius", 2.0f);
        m_B = propList.getFloat("B", 1.0f / 3.0f);
        m_C = propList.getFloat("C", 1.0f / 3.0f);
    }
    float eval(float x) const {
        x = std::abs(2.0f * x / m_radius);
        float x2 = x * x, x3 = x2 * x;
        if (x < 1) return 1.0f / 6.0f * ((12 - 9 * m_B - 6 * m_C) * x3 + (-18 + 12 * m_B + 6 * m_C) * x2 + (6 - 2 * m_B));
        if (x < 2) return 1.0f / 6.0f * ((-m_B - 6 * m_C) * x3 + (6 * m_B + 30 * m_C) * x2 + (-12 * m_B - 48 * m_C) * x + (8 * m_B + 24 * m_C));
        return 0.0f;
    }
    void fill(nori_rfilter_desc &d) const { std::memset(&d, 0, sizeof(d)); d.type = NORI_RFILTER_MITCHELL; d.radius = m_radius; d.B = m_B; d.C = m_C; }
    std::string toString() const { return format("MitchellNetravaliFilter[radius=%f, B=%f, C=%f]", m_radius, m_B, m_C); }
protected:
    float m_B, m_C;
};

class TentFilter : public ReconstructionFilter {
public:
    TentFilter(const PropertyList &) { m_radius = 1.0f; }
    float eval(float x) const { return std::max(0.0f, 1.0f - std::abs(x)); }
    void fill(nori_rfilter_desc &d) const { std::memset(&d, 0, sizeof(d)); d.type = NORI_RFILTER_TENT; d.radius = m_radius; }
    std::string toString() const { return "TentFilter[]"; }
};

class BoxFilter : public ReconstructionFilter {
public:
    BoxFilter(const PropertyList &) { m_radius = 0.5f; }
    float eval(float) const { return 1.0f; }
    void fill(nori_rfilter_desc &d) const { std::memset(&d, 0, sizeof(d)); d.type = NORI_RFILTER_BOX; d.radius = m_radius; }
    std::string toString() const { return "BoxFilter[]"; }
};
NORI_REGISTER_CLASS(GaussianFilter, "gaussian");
NORI_REGISTER_CLASS(MitchellNetravaliFilter, "mitchell");
NORI_REGISTER_CLASS(TentFilter, "tent");
NORI_REGISTER_CLASS(BoxFilter, "box");

/* ================================================================= Camera */
void Camera::setParent(NoriObject *parent) {
    if (parent && parent->getClassType() == EScene) m_scene = static_cast<Scene *>(parent);
}

class PerspectiveCamera : public Camera {
public:
    PerspectiveCamera(const PropertyList &propList) {
        m_outputSize.x() = propList.getInteger("width", 1280);
        m_outputSize.y() = propList.getInteger("height", 720);
        m_cameraToWorld = propList.getTransform("toWorld", Transform());
        m_fov = propList.getFloat("fov", 30.0f);
        m_nearClip = propList.getFloat("nearClip", 1e-4f);
        m_farClip = propList.getFloat("farClip", 1e4f);
        m_apertureRadius = propList.getFloat("apertureRadius", 0.0f);
        m_focusDistance = propList.getFloat("focusDistance", 1.0f);
        if (!std::isfinite(m_apertureRadius) || m_apertureRadius < 0.0f) throw NoriException("PerspectiveCamera: apertureRadius must be finite and not negative");
        if (m_apertureRadius > 0.0f && (!std::isfinite(m_focusDistance) || !(m_focusDistance > 0.0f)))
            throw NoriException("PerspectiveCamera: a lens (apertureRadius > 0) needs a finite, positive focusDistance");
        m_rfilter = NULL;
    }
    ~PerspectiveCamera() { delete m_rfilter; }
    void activate() {
        /* projection matrices are derived on the device side of the boundary
           (nori_hip_upload_scene, src/perspective.cpp:41-68); only the default
           filter is instantiated here (src/perspective.cpp:71-73) */
        if (!m_rfilter)
            m_rfilter = static_cast<ReconstructionFilter *>(NoriObjectFactory::createInstance("gaussian", PropertyList()));
    }
    Color3f sampleRay(Ray3f &ray, const Point2f &samplePosition, const Point2f &apertureSample) const;
    void addChild(NoriObject *obj) {
        switch (obj->getClassType()) {
        case EReconstructionFilter:
            if (m_rfilter) throw NoriException("Camera: tried to register multiple reconstruction filters!");
            m_rfilter = static_cast<ReconstructionFilter *>(obj);
            break;
        default:
            throw NoriException("Camera::addChild(<%s>) is not supported!", classTypeName(obj->getClassType()));
        }
    }
    void fill(nori_camera_desc &d) const {
        d.width = m_outputSize.x(); d.height = m_outputSize.y();
        d.fov = m_fov; d.near_clip = m_nearClip; d.far_clip = m_farClip;
        std::memcpy(d.to_world, m_cameraToWorld.m, sizeof(float) * 16);
    }
    std::string toString() const {
        return format("PerspectiveCamera[\n  cameraToWorld = %s,\n  outputSize = %s,\n  fov = %f,\n  clip = [%f, %f],\n  rfilter = %s\n]",
                      indent(m_cameraToWorld.toString(), 18), m_outputSize.toString(), m_fov, m_nearClip, m_farClip,
                      indent(m_rfilter->toString()));
    }
private:
    Transform m_cameraToWorld;
    float m_fov, m_nearClip, m_farClip;
};
NORI_REGISTER_CLASS(PerspectiveCamera, "perspective");

/* ============================================================ Integrators */
void Integrator::LiBatch(const Scene *scene, const nori_ray *rays, size_t n, const uint64_t *state, const uint64_t *seq, float *rgb) const {
    Device &d = scene->device();
    d.check(nori_hip_li(d.ctx(), rays, n, state, seq, rgb), "nori_hip_li");
}
Color3f Integrator::Li(const Scene *scene, Sampler *sampler, const Ray3f &ray) const {
    nori_ray r;
    for (int i = 0; i < 3; ++i) { r.o[i] = ray.o[i]; r.d[i] = ray.d[i]; }
    r.mint = ray.mint; r.maxt = ray.maxt;
    uint64_t st, sq; sampler->forkStream(st, sq);
    float rgb[3];
    LiBatch(scene, &r, 1, &st, &sq, rgb);
    return Color3f(rgb[0], rgb[1], rgb[2]);
}

#define NORI_SIMPLE_INTEGRATOR(Cls, Enum, Label)                                                       \
    class Cls : public Integrator {                                                                    \
    public:                                                                                            \
        Cls(const PropertyList &) {}                                                                   \
        void fill(nori_integrator_desc &d) const { std::memset(&d, 0, sizeof(d)); d.type = Enum; }    \
        std::string toString() const { return Label "[]"; }                                            \
    };
NORI_SIMPLE_INTEGRATOR(NormalIntegrator, NORI_INTEGRATOR_NORMALS, "NormalIntegrator")
NORI_SIMPLE_INTEGRATOR(AOIntegrator, NORI_INTEGRATOR_AO, "AmbientOcclusion")
NORI_SIMPLE_INTEGRATOR(WhittedIntegrator, NORI_INTEGRATOR_WHITTED, "WhittedIntegrator")
NORI_SIMPLE_INTEGRATOR(PathMatsIntegrator, NORI_INTEGRATOR_PATH_MATS, "PathMatsIntegrator")
NORI_SIMPLE_INTEGRATOR(PathEmsIntegrator, NORI_INTEGRATOR_PATH_EMS, "PathEmsIntegrator")
NORI_SIMPLE_INTEGRATOR(PathMisIntegrator, NORI_INTEGRATOR_PATH_MIS, "PathMisIntegrator")

class SimpleIntegrator : public Integrator {
public:
    SimpleIntegrator(const PropertyList &propList) {
        m_position = propList.getPoint("position");
        m_energy = propList.getColor("energy");
    }
    void fill(nori_integrator_desc &d) const {
        std::memset(&d, 0, sizeof(d)); d.type = NORI_INTEGRATOR_SIMPLE;
        for (int i = 0; i < 3; ++i) { d.position[i] = m_position[i]; d.energy[i] = m_energy[i]; }
    }
    std::string toString() const { return format("SimpleIntegrator[\n  position = %s,\n  energy = %s\n]", m_position.toString(), m_energy.toString()); }
private:
    Point3f m_position;
    Color3f m_energy;
};
NORI_REGISTER_CLASS(NormalIntegrator, "normals");
NORI_REGISTER_CLASS(AOIntegrator, "ao");
NORI_REGISTER_CLASS(SimpleIntegrator, "simple");
NORI_REGISTER_CLASS(WhittedIntegrator, "whitted");
NORI_REGISTER_CLASS(PathMatsIntegrator, "path_mats");
NORI_REGISTER_CLASS(PathEmsIntegrator, "path_ems");
NORI_REGISTER_CLASS(PathMisIntegrator, "path_mis");

/* =================================================================== Mesh */
Mesh::Mesh() {}
Mesh::~Mesh() { delete m_bsdf; delete m_emitter; }

void Mesh::activate() {
    if (!m_bsdf)   /* src/mesh.cpp:23-29: default diffuse BRDF */
        m_bsdf = static_cast<BSDF *>(NoriObjectFactory::createInstance("diffuse", PropertyList()));
}

void Mesh::addChild(NoriObject *obj) {
    switch (obj->getClassType()) {
    case EBSDF:
        if (m_bsdf) throw NoriException("Mesh: tried to register multiple BSDF instances!");
        m_bsdf = static_cast<BSDF *>(obj);
        break;
    case EEmitter:
        if (m_emitter) throw NoriException("Mesh: tried to register multiple Emitter instances!");
        m_emitter = static_cast<Emitter *>(obj);
        break;
    default:
        throw NoriException("Mesh::addChild(<%s>) is not supported!", classTypeName(obj->getClassType()));
    }
}

std::string Mesh::toString() const {
    return format("Mesh[\n  name = \"%s\",\n  vertexCount = %i,\n  triangleCount = %i,\n  bsdf = %s,\n  emitter = %s\n]",
                  m_name, (int) getVertexCount(), (int) getTriangleCount(),
                  m_bsdf ? indent(m_bsdf->toString()) : std::string("null"),
                  m_emitter ? indent(m_emitter->toString()) : std::string("null"));
}

void Mesh::fill(nori_mesh_desc &d) const {
    std::memset(&d, 0, sizeof(d));
    d.n_vertices = getVertexCount(); d.n_triangles = getTriangleCount();
    d.positions = m_V.data();
    d.normals = m_N.empty() ? nullptr : m_N.data();
    d.texcoords = m_UV.empty() ? nullptr : m_UV.data();
    d.indices = m_F.data();
    m_bsdf->fill(d.bsdf);
    d.is_emitter = m_emitter ? 1 : 0;
    if (m_emitter) { Color3f r = m_emitter->getRadiance(); for (int i = 0; i < 3; ++i) d.radiance[i] = r[i]; }
}

std::string Intersection::toString() const {
    if (!mesh) return "Intersection[invalid]";
    return format("Intersection[\n  p = %s,\n  t = %f,\n  uv = %s,\n  mesh = %s\n]", p.toString(), t, uv.toString(), mesh->getName());
}

/* ================================================================== Accel */
void Accel::addMesh(Mesh *mesh) { m_meshes.push_back(mesh); }

void Accel::build() {
    /* Accel::build of the reference is a no-op (src/accel.cpp:19-21).  Here it
       is where the BVH comes from -- but the build runs on the far side of the
       C ABI, the first time the scene's device context is requested
       (Scene::device), so that a scene can be parsed and flattened on a
       machine without a GPU. */
}

static void toRay(const Ray3f &ray, nori_ray &r) {
    for (int i = 0; i < 3; ++i) { r.o[i] = ray.o[i]; r.d[i] = ray.d[i]; }
    r.mint = ray.mint; r.maxt = ray.maxt;
}

void Accel::rayIntersectBatch(const nori_ray *rays, nori_intersection *its, size_t n, bool shadowRay) const {
    Device &d = m_scene->device();
    d.check(nori_hip_intersect(d.ctx(), rays, its, n, shadowRay ? 1 : 0), "nori_hip_intersect");
}

bool Accel::rayIntersect(const Ray3f &ray, Intersection &its, bool shadowRay) const {
    nori_ray r; toRay(ray, r);
    nori_intersection o;
    rayIntersectBatch(&r, &o, 1, shadowRay);
    if (o.mesh == NORI_NO_HIT) return false;
    if (shadowRay) return true;
    its.p = Point3f(o.p[0], o.p[1], o.p[2]); its.t = o.t; its.uv = Point2f(o.uv[0], o.uv[1]);
    its.shFrame.s = Vector3f(o.sh_s[0], o.sh_s[1], o.sh_s[2]); its.shFrame.t = Vector3f(o.sh_t[0], o.sh_t[1], o.sh_t[2]);
    its.shFrame.n = Vector3f(o.sh_n[0], o.sh_n[1], o.sh_n[2]);
    its.geoFrame.s = Vector3f(o.geo_s[0], o.geo_s[1], o.geo_s[2]); its.geoFrame.t = Vector3f(o.geo_t[0], o.geo_t[1], o.geo_t[2]);
    its.geoFrame.n = Vector3f(o.geo_n[0], o.geo_n[1], o.geo_n[2]);
    its.mesh = m_meshes[o.mesh]; its.tri = o.tri;
    return true;
}

Color3f PerspectiveCamera::sampleRay(Ray3f &ray, const Point2f &samplePosition, const Point2f &apertureSample) const {
    if (!m_scene) throw NoriException("PerspectiveCamera::sampleRay(): the camera is not attached to a scene");
    Device &d = m_scene->device();
    nori_ray r;
    /* (the context's lens is this camera's: Scene::device; without one the bits of nori_hip_sample_rays) */
    d.check(nori_hip_sample_rays_lens(d.ctx(), samplePosition.v, apertureSample.v, 1, &r), "nori_hip_sample_rays_lens");
    ray.o = Point3f(r.o[0], r.o[1], r.o[2]); ray.d = Vector3f(r.d[0], r.d[1], r.d[2]);
    ray.mint = r.mint; ray.maxt = r.maxt; ray.update();
    return Color3f(1.0f);
}

/* ================================================================== Scene */
bool Scene::s_verbose = true;

Scene::Scene(const PropertyList &) { m_accel = new Accel(this); std::memset(&m_desc, 0, sizeof(m_desc)); }

Scene::~Scene() {
    delete m_accel; delete m_sampler; delete m_camera; delete m_integrator; delete m_environment; delete m_medium;
    for (Mesh *m : m_meshes) delete m;       /* the reference leaks these (src/scene.cpp:20-25) */
    for (Emitter *e : m_lightObjects) delete e;
}

void Scene::activate() {
    m_accel->build();
    if (!m_integrator) throw NoriException("No integrator was specified!");
    if (!m_camera) throw NoriException("No camera was specified!");
    if (m_environment) {      /* what nori_hip_set_environment would refuse, said before a device is asked for */
        nori_integrator_desc id;
        m_integrator->fill(id);
        if (id.type == NORI_INTEGRATOR_WHITTED)
            throw NoriException("An environment map cannot be rendered by the whitted integrator (use path_mats, path_ems or path_mis)");
    }
    if (m_medium) {           /* what nori_hip_set_medium would refuse, likewise */
        nori_integrator_desc id;
        m_integrator->fill(id);
        if (id.type != NORI_INTEGRATOR_PATH_MATS && id.type != NORI_INTEGRATOR_PATH_EMS && id.type != NORI_INTEGRATOR_PATH_MIS)
            throw NoriException("A medium is rendered by path_mats, path_ems and path_mis only");
        if (m_environment && m_medium->isGrid())
            throw NoriException("A grid medium cannot be lit by an environment map yet (no kernel set combines the two)");
        if (m_environment)
            throw NoriException("A medium that fills all space cannot be lit by an environment map (its transmittance to infinity is zero)");
    }
    if (!m_lights.empty()) {  /* what nori_hip_set_lights would refuse, likewise */
        nori_integrator_desc id;
        m_integrator->fill(id);
        if (id.type != NORI_INTEGRATOR_PATH_EMS && id.type != NORI_INTEGRATOR_PATH_MIS)
            throw NoriException("Point, spot and directional lights are rendered by path_ems and path_mis only");
        if (m_lights.size() > NORI_MAX_LIGHTS) throw NoriException("There can be at most %d point, spot and directional lights per scene!", (int) NORI_MAX_LIGHTS);
        if (m_medium && !m_medium->isGrid())      /* (a grid medium is bounded by its box: a directional light may light it) */
            for (const nori_light_desc &l : m_lights)
                if (l.type == NORI_LIGHT_DIRECTIONAL)
                    throw NoriException("A directional light cannot light a medium that fills all space (its transmittance from infinity is zero)");
    }
    if (!m_sampler)
        m_sampler = static_cast<Sampler *>(NoriObjectFactory::createInstance("independent", PropertyList()));
    if (s_verbose) {
        cout << endl;
        cout << "Configuration: " << toString() << endl;
        cout << endl;
    }
}

void Scene::addChild(NoriObject *obj) {
    switch (obj->getClassType()) {
    case EMesh: {
        Mesh *mesh = static_cast<Mesh *>(obj);
        m_accel->addMesh(mesh);
        m_meshes.push_back(mesh);
    } break;
    case EEmitter:
        /* src/scene.cpp:55-59 throws here: the reference attaches emitters to meshes.  An environment map is the one emitter
           that belongs to the scene (a departure: INTEGRATION.md) */
        if (static_cast<Emitter *>(obj)->isDeltaLight()) {      /* (likewise a departure: lights without geometry) */
            m_lights.emplace_back();
            static_cast<Emitter *>(obj)->fillLight(m_lights.back());
            m_lightObjects.push_back(static_cast<Emitter *>(obj));
            break;
        }
        if (!static_cast<Emitter *>(obj)->isEnvironment())
            throw NoriException("Scene::addChild(): emitters must be children of a <mesh> (area lights); only <emitter type=\"envmap\"> and point, spot and directional lights belong to the scene");
        if (m_environment) throw NoriException("There can only be one environment map per scene!");
        m_environment = static_cast<Emitter *>(obj);
        break;
    case EMedium:
        if (m_medium) throw NoriException("There can only be one medium per scene!");
        m_medium = static_cast<Medium *>(obj);
        break;
    case ESampler:
        if (m_sampler) throw NoriException("There can only be one sampler per scene!");
        m_sampler = static_cast<Sampler *>(obj);
        break;
    case ECamera:
        if (m_camera) throw NoriException("There can only be one camera per scene!");
        m_camera = static_cast<Camera *>(obj);
        break;
    case EIntegrator:
        if (m_integrator) throw NoriException("There can only be one integrator per scene!");
        m_integrator = static_cast<Integrator *>(obj);
        break;
    default:
        throw NoriException("Scene::addChild(<%s>) is not supported!", classTypeName(obj->getClassType()));
    }
    m_descValid = false;
}

std::string Scene::toString() const {
    std::string meshes;
    for (size_t i = 0; i < m_meshes.size(); ++i) {
        meshes += std::string("  ") + indent(m_meshes[i]->toString(), 2);
        if (i + 1 < m_meshes.size()) meshes += ",";
        meshes += "\n";
    }
    return format("Scene[\n  integrator = %s,\n  sampler = %s\n  camera = %s,\n  meshes = {\n  %s  }\n]",
                  indent(m_integrator->toString()), indent(m_sampler->toString()), indent(m_camera->toString()), indent(meshes, 2));
}

const nori_scene_desc &Scene::getDesc() const {
    if (!m_descValid) {
        m_meshDescs.resize(m_meshes.size());
        for (size_t i = 0; i < m_meshes.size(); ++i) m_meshes[i]->fill(m_meshDescs[i]);
        std::memset(&m_desc, 0, sizeof(m_desc));
        m_desc.n_meshes = (uint32_t) m_meshes.size();
        m_desc.meshes = m_meshDescs.data();
        m_camera->fill(m_desc.camera);
        m_camera->getReconstructionFilter()->fill(m_desc.rfilter);
        m_integrator->fill(m_desc.integrator);
        m_desc.sample_count = (int32_t) m_sampler->getSampleCount();
        /* albedo textures: one record per texture object, referenced 1-based by the meshes (the objects own the texels) */
        std::vector<const Texture *> textures;
        m_textureDescs.clear();
        for (size_t i = 0; i < m_meshes.size(); ++i) {
            const Texture *t = m_meshes[i]->getBSDF()->albedoTexture();
            if (!t) continue;
            size_t k = std::find(textures.begin(), textures.end(), t) - textures.begin();
            if (k == textures.size()) { textures.push_back(t); m_textureDescs.emplace_back(); t->fill(m_textureDescs.back()); }
            m_meshDescs[i].albedo_texture = (uint32_t) k + 1u;
        }
        m_desc.n_textures = (uint32_t) m_textureDescs.size();
        m_desc.textures = m_textureDescs.empty() ? nullptr : m_textureDescs.data();
        m_descValid = true;
    }
    return m_desc;
}

Device &Scene::device() const {
    if (!m_device) {
        std::unique_ptr<Device> d(new Device());
        const nori_scene_desc &desc = getDesc();
        d->check(nori_hip_upload_scene(d->ctx(), &desc), "nori_hip_upload_scene");
        d->check(nori_hip_build_accel(d->ctx(), NORI_ACCEL_AUTO), "nori_hip_build_accel");
        if (m_camera->getApertureRadius() > 0.0f)      /* (the upload leaves the pinhole) */
            d->check(nori_hip_set_lens(d->ctx(), m_camera->getApertureRadius(), m_camera->getFocusDistance()), "nori_hip_set_lens");
        if (m_environment) {      /* (nor an environment) */
            nori_env_desc env;
            m_environment->fillEnvironment(env);
            d->check(nori_hip_set_environment(d->ctx(), &env), "nori_hip_set_environment");
        }
        if (m_medium && m_medium->isGrid()) {
            nori_grid_medium_desc gd;
            m_medium->fillGridMedium(gd);
            d->check(nori_hip_set_grid_medium(d->ctx(), &gd), "nori_hip_set_grid_medium");
        } else if (m_medium) {
            nori_medium_desc md;
            m_medium->fillMedium(md);
            d->check(nori_hip_set_medium(d->ctx(), &md), "nori_hip_set_medium");
        }
        if (!m_lights.empty()) d->check(nori_hip_set_lights(d->ctx(), (uint32_t) m_lights.size(), m_lights.data()), "nori_hip_set_lights");
        m_device = std::move(d);
    }
    return *m_device;
}
DeviceGroup &Scene::deviceGroup(int n) const {
    if (!m_group || m_group->size() != n) {
        std::unique_ptr<DeviceGroup> g(new DeviceGroup(n));
        const nori_scene_desc &desc = getDesc();
        g->check(nori_hip_group_upload_scene(g->group(), &desc, NORI_ACCEL_AUTO), "nori_hip_group_upload_scene");
        if (m_camera->getApertureRadius() > 0.0f)
            g->check(nori_hip_group_set_lens(g->group(), m_camera->getApertureRadius(), m_camera->getFocusDistance()), "nori_hip_group_set_lens");
        if (m_environment) {
            nori_env_desc env;
            m_environment->fillEnvironment(env);
            g->check(nori_hip_group_set_environment(g->group(), &env), "nori_hip_group_set_environment");
        }
        if (m_medium && m_medium->isGrid()) {
            nori_grid_medium_desc gd;
            m_medium->fillGridMedium(gd);
            g->check(nori_hip_group_set_grid_medium(g->group(), &gd), "nori_hip_group_set_grid_medium");
        } else if (m_medium) {
            nori_medium_desc md;
            m_medium->fillMedium(md);
            g->check(nori_hip_group_set_medium(g->group(), &md), "nori_hip_group_set_medium");
        }
        if (!m_lights.empty()) g->check(nori_hip_group_set_lights(g->group(), (uint32_t) m_lights.size(), m_lights.data()), "nori_hip_group_set_lights");
        m_group = std::move(g);
    }
    return *m_group;
}
void Scene::setLens(float radius, float focusDistance) {
    if (!m_camera) throw NoriException("Scene::setLens(): no camera");
    m_camera->setLens(radius, focusDistance);
    if (m_device) m_device->check(nori_hip_set_lens(m_device->ctx(), radius, focusDistance), "nori_hip_set_lens");
    if (m_group) m_group->check(nori_hip_group_set_lens(m_group->group(), radius, focusDistance), "nori_hip_group_set_lens");
}
NORI_REGISTER_CLASS(Scene, "scene");

NORI_NAMESPACE_END
