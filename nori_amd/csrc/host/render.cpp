/*
 * render.cpp -- ImageBlock (host view) and the render driver.
 *
 * renderScene() stands where render() of the reference's src/main.cpp:58-148
 * does: instead of tbb::parallel_for over 32x32 blocks calling renderBlock
 * (main.cpp:27-56) per block, one call hands the whole frame to
 * nori_hip_render -- block scheduling, sampling, Li and the filtered splat all
 * run in the render kernel -- and the full-frame RGBW block comes back for
 * toBitmap (src/block.cpp:45-51).
 *
 * NORI_GPUS=N in the environment (`nori scene.xml --gpus N`) shares the frame over the first N GPUs of the node: the
 * blocks the reference's parallel_for hands to TBB workers (src/main.cpp:85-113) go to devices -- 16x16 tiles round
 * robin (NORI_SPLIT=tile, default) or a range of the sample indices each (NORI_SPLIT=sample) -- and the mutex-guarded
 * ImageBlock::put(ImageBlock&) (src/block.cpp:93-102) becomes one RCCL merge on the first device (NORI_MERGE=reduce,
 * default, or gather): nori_hip_group_render_host, one host thread and one context per device inside the library.
 */
#include <nori/bitmap.h>
#include <nori/plugins.h>

NORI_NAMESPACE_BEGIN

ImageBlock::ImageBlock(const Vector2i &size, const ReconstructionFilter *filter) : m_offset(0, 0), m_size(size) {
    if (filter) m_borderSize = (int) std::ceil(filter->getRadius() - 0.5f);     /* src/block.cpp:20 */
    m_data.assign((size_t) rows() * cols() * 4, 0.0f);
}

Bitmap *ImageBlock::toBitmap() const {
    Bitmap *result = new Bitmap(m_size);
    for (int y = 0; y < m_size.y(); ++y)
        for (int x = 0; x < m_size.x(); ++x) {
            const float *p = &m_data[((size_t) (y + m_borderSize) * cols() + (x + m_borderSize)) * 4];
            /* Color4f::divideByFilterWeight, include/nori/color.h:100-105 */
            if (p[3] != 0) result->set(y, x, Color3f(p[0] / p[3], p[1] / p[3], p[2] / p[3]));
            else result->set(y, x, Color3f(0.0f));
        }
    return result;
}

void ImageBlock::put(const ImageBlock &b) {
    if (b.rows() != rows() || b.cols() != cols()) throw NoriException("ImageBlock::put(): block sizes differ");
    for (size_t i = 0; i < m_data.size(); ++i) m_data[i] += b.m_data[i];
}

std::string ImageBlock::toString() const { return format("ImageBlock[offset=%s, size=%s]]", m_offset.toString(), m_size.toString()); }

std::unique_ptr<ImageBlock> renderScene(Scene *scene, nori_render_stats *stats) {
    const Camera *camera = scene->getCamera();
    scene->getIntegrator()->preprocess(scene);
    std::unique_ptr<ImageBlock> result(new ImageBlock(camera->getOutputSize(), camera->getReconstructionFilter()));
    result->clear();

    nori_render_params params;
    std::memset(&params, 0, sizeof(params));
    params.spp_begin = 0;
    params.spp_count = (uint32_t) scene->getSampler()->getSampleCount();
    params.tile_mod = 1; params.tile_rem = 0;
    /* sampler streams: one pcg32 stream per camera sample (default), or -- NORI_SEED=block in the environment, `--seed block`
       on the nori command line -- the reference's own scheme, one serial stream per 32x32 block seeded by
       Independent::prepare (src/independent.cpp:36-41), which the device then runs one lane per block */
    const char *seed = std::getenv("NORI_SEED");
    params.seed_mode = (seed && std::string(seed) == "block") ? NORI_SEED_NORI_BLOCK : NORI_SEED_PER_SAMPLE;
    nori_render_stats local;
    if (const char *gpus = std::getenv("NORI_GPUS")) {
        const int n = std::atoi(gpus);
        if (n < 1) throw NoriException("NORI_GPUS / --gpus expects a positive number of GPUs, got \"%s\"", gpus);
        const char *sp = std::getenv("NORI_SPLIT"), *mg = std::getenv("NORI_MERGE");
        const std::string split = sp ? sp : "tile", merge = mg ? mg : "reduce";
        if (split != "tile" && split != "sample") throw NoriException("NORI_SPLIT / --split expects \"tile\" or \"sample\", got \"%s\"", split);
        if (merge != "reduce" && merge != "gather") throw NoriException("NORI_MERGE / --merge expects \"reduce\" or \"gather\", got \"%s\"", merge);
        DeviceGroup &grp = scene->deviceGroup(n);
        float merge_ms = 0.0f;
        grp.check(nori_hip_group_render_host(grp.group(), &params, split == "sample" ? NORI_SPLIT_SAMPLE : NORI_SPLIT_TILE,
                                             merge == "gather" ? NORI_MERGE_GATHER : NORI_MERGE_REDUCE, camera->getOutputSize().x(), camera->getOutputSize().y(),
                                             result->data(), stats ? stats : &local, &merge_ms), "nori_hip_group_render_host");
        if (Scene::s_verbose) cout << "[" << n << " GPUs, " << split << " split, " << merge << " merge over " << nori_hip_group_transport(grp.group()) << ": " << merge_ms << " ms] ";
        return result;
    }
    Device &dev = scene->device();          /* uploads the scene and builds the BVH on first use */
    dev.check(nori_hip_render_host(dev.ctx(), &params, result->data(), stats ? stats : &local), "nori_hip_render_host");
    return result;
}

std::unique_ptr<ImageBlock> renderSceneToError(Scene *scene, float targetError, uint32_t passSpp, uint32_t &sppDone,
                                               nori_error_summary &summary, std::vector<float> &errorMap, nori_render_stats *stats) {
    const Camera *camera = scene->getCamera();
    scene->getIntegrator()->preprocess(scene);
    if (const char *gpus = std::getenv("NORI_GPUS"))
        if (std::atoi(gpus) > 1) throw NoriException("--target-error renders on one device: moment frames over a device group are not supported (got --gpus %s)", gpus);
    if (const char *seed = std::getenv("NORI_SEED"))
        if (std::string(seed) == "block") throw NoriException("--target-error renders in passes, which --seed block cannot (a block's stream is serial from sample 0)");
    std::unique_ptr<ImageBlock> result(new ImageBlock(camera->getOutputSize(), camera->getReconstructionFilter()));
    result->clear();
    errorMap.assign((size_t) camera->getOutputSize().x() * camera->getOutputSize().y(), 0.0f);

    nori_render_params params;
    std::memset(&params, 0, sizeof(params));
    params.spp_begin = 0;
    params.spp_count = (uint32_t) scene->getSampler()->getSampleCount();      /* the ceiling */
    params.tile_mod = 1; params.tile_rem = 0;
    params.seed_mode = NORI_SEED_PER_SAMPLE;
    nori_render_stats local;
    Device &dev = scene->device();
    dev.check(nori_hip_render_to_error_host(dev.ctx(), &params, passSpp, targetError, result->data(), nullptr, errorMap.data(), &sppDone, &summary,
                                            stats ? stats : &local), "nori_hip_render_to_error_host");
    return result;
}

std::unique_ptr<ImageBlock> renderSceneAdaptive(Scene *scene, float targetError, uint32_t passSpp, nori_adaptive_summary &summary,
                                                std::vector<float> &errorMap, std::vector<uint32_t> &tileSpp, nori_render_stats *stats,
                                                const nori_allocate_params *allocate) {
    const Camera *camera = scene->getCamera();
    scene->getIntegrator()->preprocess(scene);
    if (const char *gpus = std::getenv("NORI_GPUS"))
        if (std::atoi(gpus) > 1) throw NoriException("--target-error renders on one device: moment frames over a device group are not supported (got --gpus %s)", gpus);
    if (const char *seed = std::getenv("NORI_SEED"))
        if (std::string(seed) == "block") throw NoriException("--target-error renders in passes, which --seed block cannot (a block's stream is serial from sample 0)");
    std::unique_ptr<ImageBlock> result(new ImageBlock(camera->getOutputSize(), camera->getReconstructionFilter()));
    result->clear();
    const int w = camera->getOutputSize().x(), h = camera->getOutputSize().y();
    errorMap.assign((size_t) w * h, 0.0f);
    tileSpp.assign((size_t) ((w + NORI_TILE_SIZE - 1) / NORI_TILE_SIZE) * ((h + NORI_TILE_SIZE - 1) / NORI_TILE_SIZE), 0u);

    nori_render_params params;
    std::memset(&params, 0, sizeof(params));
    params.spp_begin = 0;
    params.spp_count = (uint32_t) scene->getSampler()->getSampleCount();      /* the most a pixel may get */
    params.tile_mod = 1; params.tile_rem = 0;
    params.seed_mode = NORI_SEED_PER_SAMPLE;
    nori_render_stats local;
    Device &dev = scene->device();
    if (allocate)
        dev.check(nori_hip_render_allocated_host(dev.ctx(), &params, allocate, nullptr, result->data(), nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr,
                                                 errorMap.data(), tileSpp.data(), nullptr, &summary, stats ? stats : &local), "nori_hip_render_allocated_host");
    else
        dev.check(nori_hip_render_adaptive_host(dev.ctx(), &params, passSpp, targetError, result->data(), nullptr, errorMap.data(), tileSpp.data(), &summary,
                                                stats ? stats : &local), "nori_hip_render_adaptive_host");
    return result;
}

void renderSceneFeatures(Scene *scene, uint32_t spp, std::vector<float> &albedo, std::vector<float> &normal, std::vector<float> &depth,
                         int &border, nori_render_stats *stats) {
    const Camera *camera = scene->getCamera();
    if (const char *gpus = std::getenv("NORI_GPUS"))
        if (std::atoi(gpus) > 1) throw NoriException("--features renders on one device: feature frames over a device group are not supported (got --gpus %s)", gpus);
    ImageBlock shape(camera->getOutputSize(), camera->getReconstructionFilter());      /* the frames' layout */
    border = shape.getBorderSize();
    const size_t n = (size_t) shape.rows() * shape.cols() * 4;
    albedo.assign(n, 0.0f); normal.assign(n, 0.0f); depth.assign(n, 0.0f);

    nori_render_params params;
    std::memset(&params, 0, sizeof(params));
    params.spp_begin = 0;
    params.spp_count = spp;
    params.tile_mod = 1; params.tile_rem = 0;
    params.seed_mode = NORI_SEED_PER_SAMPLE;
    nori_render_stats local;
    Device &dev = scene->device();          /* the context of the beauty render: the scene is uploaded and the tree built */
    dev.check(nori_hip_render_features_host(dev.ctx(), &params, NORI_FEATURE_ALBEDO | NORI_FEATURE_NORMAL | NORI_FEATURE_DEPTH, albedo.data(), normal.data(),
                                            depth.data(), stats ? stats : &local), "nori_hip_render_features_host");
}

std::unique_ptr<ImageBlock> renderSceneDenoised(Scene *scene, const nori_denoise_params &dn, uint32_t featureSpp, std::vector<float> &denoised,
                                                nori_render_stats *stats) {
    const Camera *camera = scene->getCamera();
    scene->getIntegrator()->preprocess(scene);
    if (const char *gpus = std::getenv("NORI_GPUS"))
        if (std::atoi(gpus) > 1) throw NoriException("--denoise renders on one device: moment and feature frames over a device group are not supported (got --gpus %s)", gpus);
    if (const char *seed = std::getenv("NORI_SEED"))
        if (std::string(seed) == "block") throw NoriException("--denoise needs the feature frames, which --seed block cannot give (a block's stream is serial)");
    std::unique_ptr<ImageBlock> result(new ImageBlock(camera->getOutputSize(), camera->getReconstructionFilter()));
    result->clear();
    std::vector<float> m2((size_t) result->rows() * result->cols() * 4, 0.0f);

    nori_render_params params;
    std::memset(&params, 0, sizeof(params));
    params.spp_begin = 0;
    params.spp_count = (uint32_t) scene->getSampler()->getSampleCount();
    params.tile_mod = 1; params.tile_rem = 0;
    params.seed_mode = NORI_SEED_PER_SAMPLE;
    nori_render_stats local;
    Device &dev = scene->device();
    dev.check(nori_hip_render_moments_host(dev.ctx(), &params, result->data(), m2.data(), stats ? stats : &local), "nori_hip_render_moments_host");
    std::vector<float> fa, fn, fd;
    int border = 0;
    renderSceneFeatures(scene, featureSpp, fa, fn, fd, border);
    const size_t n = (size_t) camera->getOutputSize().x() * camera->getOutputSize().y();
    denoised.assign(n * 3, 0.0f);
    dev.check(nori_hip_denoise_host(dev.ctx(), &dn, result->data(), m2.data(), fa.data(), fn.data(), fd.data(), denoised.data(), nullptr), "nori_hip_denoise_host");
    return result;
}

std::unique_ptr<ImageBlock> renderSceneAdaptiveDenoised(Scene *scene, float targetError, uint32_t passSpp, const nori_denoise_params &dn, uint32_t featureSpp,
                                                        nori_adaptive_summary &summary, std::vector<float> &denoised, std::vector<float> &errorMap,
                                                        std::vector<uint32_t> &tileSpp, nori_render_stats *stats, const nori_allocate_params *allocate) {
    const Camera *camera = scene->getCamera();
    scene->getIntegrator()->preprocess(scene);
    if (const char *gpus = std::getenv("NORI_GPUS"))
        if (std::atoi(gpus) > 1) throw NoriException("--target-denoised-error renders on one device: moment and feature frames over a device group are not supported (got --gpus %s)", gpus);
    if (const char *seed = std::getenv("NORI_SEED"))
        if (std::string(seed) == "block") throw NoriException("--target-denoised-error renders in passes, which --seed block cannot (a block's stream is serial from sample 0)");
    std::unique_ptr<ImageBlock> result(new ImageBlock(camera->getOutputSize(), camera->getReconstructionFilter()));
    result->clear();
    const int w = camera->getOutputSize().x(), h = camera->getOutputSize().y();
    const size_t n = (size_t) w * h;
    denoised.assign(n * 3, 0.0f);
    errorMap.assign(n, 0.0f);
    tileSpp.assign((size_t) ((w + NORI_TILE_SIZE - 1) / NORI_TILE_SIZE) * ((h + NORI_TILE_SIZE - 1) / NORI_TILE_SIZE), 0u);
    std::vector<float> fa, fn, fd;
    int border = 0;
    renderSceneFeatures(scene, featureSpp, fa, fn, fd, border);      /* first: the loop is guided by them from its second pass on */

    nori_render_params params;
    std::memset(&params, 0, sizeof(params));
    params.spp_begin = 0;
    params.spp_count = (uint32_t) scene->getSampler()->getSampleCount();      /* the most a pixel may get */
    params.tile_mod = 1; params.tile_rem = 0;
    params.seed_mode = NORI_SEED_PER_SAMPLE;
    nori_render_stats local;
    Device &dev = scene->device();
    if (allocate)
        dev.check(nori_hip_render_allocated_host(dev.ctx(), &params, allocate, &dn, result->data(), nullptr, fa.data(), fn.data(), fd.data(), denoised.data(), nullptr,
                                                 nullptr, errorMap.data(), tileSpp.data(), nullptr, &summary, stats ? stats : &local), "nori_hip_render_allocated_host");
    else
        dev.check(nori_hip_render_adaptive_denoised_host(dev.ctx(), &params, passSpp, targetError, &dn, result->data(), nullptr, fa.data(), fn.data(), fd.data(),
                                                         denoised.data(), nullptr, nullptr, errorMap.data(), tileSpp.data(), &summary, stats ? stats : &local),
                  "nori_hip_render_adaptive_denoised_host");
    return result;
}

NORI_NAMESPACE_END
