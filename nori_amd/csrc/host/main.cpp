/*
 * main.cpp -- `nori <scene.xml> [--no-gui] [--threads N] [--seed sample|block] [--gpus N] [--split tile|sample] [--merge reduce|gather] [--film-order fast|reference] [--aperture R] [--focus-distance F | --focus-pixel X Y] [--target-error E [--pass-spp K] [--adaptive]] [--features [--feature-spp K]] [--denoise [--denoise-radius R] [--denoise-patch F]] [--target-denoised-error E [--pass-spp K] [--feature-spp K] [--denoise-radius R] [--denoise-patch F]] [--allocate [--pilot-spp K] [--rounds N]]`
 * Command line of the reference (src/main.cpp:150-246).  There is no GUI on a
 * compute node: --no-gui is accepted and implied; --threads is accepted for
 * compatibility (the work runs on the GPU).  --seed block renders with the
 * reference's sampler streams (one pcg32 stream per 32x32 block,
 * src/independent.cpp:36-41; one GPU lane per block, slow by design) instead of
 * one stream per camera sample.  --gpus N shares the frame over the first N GPUs
 * of the node (render.cpp: what TBB workers are in the reference; --split / --merge
 * choose how the work is cut and how the frames come together).  --target-error E renders
 * in passes of K samples per pixel (--pass-spp, default 16) until the mean of the per-pixel
 * error map (include/nori_hip.h: nori_hip_error_map) is at most E, the scene's sampleCount
 * being the most it spends; it prints where it stopped and writes the map as
 * <scene>.error.exr next to the frame (one device only).  With --adaptive a pass renders only
 * the 16x16 tiles whose mean error is still above E (nori_hip_render_adaptive); the samples
 * every pixel's tile received are written as <scene>.spp.exr.  --features runs, after the render and
 * on the same context, the first-hit feature pass (nori_hip_render_features) over camera samples
 * [0, K) of every pixel -- K = --feature-spp, default min(sampleCount, 16): the beauty frame's own
 * first K sample positions -- and writes <scene>.albedo.exr, <scene>.normal.exr (decoded to
 * [-1, 1], not renormalised) and <scene>.depth.exr (mean distance over the hits, coverage, mean
 * squared distance), one device only.  --denoise renders through nori_hip_render_moments, renders the
 * three feature frames with the scene's sample count (or --feature-spp), runs nori_hip_denoise over
 * them -- window radius --denoise-radius (1..8, default 5), patch radius --denoise-patch (0..2,
 * default 1) -- and writes <scene>.denoised.exr beside the usual output; one device only, not
 * together with --target-error.  --target-denoised-error E renders the three feature frames first (K = --feature-spp, default
 * min(sampleCount, 16)), then runs nori_hip_render_adaptive_denoised: passes of --pass-spp samples per pixel over the 16x16 tiles
 * whose DENOISED error (nori_hip_denoised_tile_errors) is still above E, the scene's sampleCount being the most a pixel gets.  It
 * writes the usual output (the raw frame), <scene>.denoised.exr, <scene>.error.exr (the denoised error map) and <scene>.spp.exr and
 * prints where it stopped; one device only, not together with --denoise, --target-error or --adaptive.  --allocate modifies --target-error E
 * and --target-denoised-error E: instead of passes of --pass-spp samples, a pilot of K samples per pixel (--pilot-spp, default 16) and at
 * most N rounds (--rounds, default 3) that render every tile still above E up to the level K << j its error predicts, one render per
 * group of tiles that share a move (nori_hip_render_allocated); it writes the files of those modes, <scene>.error.exr and
 * <scene>.spp.exr included; one device only, not together with --adaptive.  A <test> root runs during parsing
 * (its activate()), as in the reference; failures exit with -1.
 */
#include <nori/bitmap.h>
#include <nori/plugins.h>

using namespace nori;

int main(int argc, char **argv) {
    if (argc < 2) {
        cerr << "Syntax: " << argv[0] << " <scene.xml> [--no-gui] [--threads N] [--seed sample|block] [--gpus N] [--split tile|sample] [--merge reduce|gather] [--film-order fast|reference] [--aperture R] [--focus-distance F | --focus-pixel X Y] [--target-error E [--pass-spp K] [--adaptive]] [--features [--feature-spp K]] [--denoise [--denoise-radius R] [--denoise-patch F]] [--target-denoised-error E [--pass-spp K] [--feature-spp K] [--denoise-radius R] [--denoise-patch F]] [--allocate [--pilot-spp K] [--rounds N]]" << endl;
        return -1;
    }
    std::string sceneName;
    bool toError = false, havePassSpp = false, adaptive = false, features = false, haveFeatureSpp = false;
    long featureSpp = 16;
    bool denoise = false, haveDenoiseRadius = false, haveDenoisePatch = false;
    bool toDenoisedError = false;
    bool allocate = false, havePilotSpp = false, haveRounds = false;
    long pilotSpp = 16, rounds = 3;
    long denoiseRadius = 5, denoisePatch = 1;
    float targetError = 0.0f;
    long passSpp = 16;
    int gpus = 1;
    bool haveAperture = false, haveFocusDistance = false, haveFocusPixel = false;      /* the thin lens: override the camera's apertureRadius / focusDistance */
    float aperture = 0.0f, focusDistance = 1.0f;
    long focusPixel[2] = {0, 0};
    for (int i = 1; i < argc; ++i) {
        std::string token(argv[i]);
        if (token == "-t" || token == "--threads") {
            if (i + 1 >= argc || atoi(argv[i + 1]) <= 0) {
                cerr << "\"--threads\" argument expects a positive integer following it." << endl;
                return -1;
            }
            ++i;
            continue;
        } else if (token == "--no-gui") {
            continue;
        } else if (token == "--seed") {
            if (i + 1 >= argc || (std::string(argv[i + 1]) != "sample" && std::string(argv[i + 1]) != "block")) {
                cerr << "\"--seed\" expects \"sample\" or \"block\"." << endl;
                return -1;
            }
            setenv("NORI_SEED", argv[++i], 1);
            continue;
        } else if (token == "--gpus") {
            if (i + 1 >= argc || atoi(argv[i + 1]) <= 0) {
                cerr << "\"--gpus\" argument expects a positive integer following it." << endl;
                return -1;
            }
            gpus = atoi(argv[i + 1]);
            setenv("NORI_GPUS", argv[++i], 1);
            continue;
        } else if (token == "--target-error") {
            char *end = nullptr;
            if (i + 1 < argc) targetError = std::strtof(argv[i + 1], &end);
            if (i + 1 >= argc || end == argv[i + 1] || *end != '\0' || !(targetError >= 0.0f) || std::isinf(targetError)) {
                cerr << "Usage: \"--target-error\" expects a mean relative error >= 0 following it, e.g. --target-error 0.05 [--pass-spp K]." << endl;
                return -1;
            }
            toError = true; ++i;
            continue;
        } else if (token == "--target-denoised-error") {
            char *end = nullptr;
            if (i + 1 < argc) targetError = std::strtof(argv[i + 1], &end);
            if (i + 1 >= argc || end == argv[i + 1] || *end != '\0' || !(targetError >= 0.0f) || std::isinf(targetError)) {
                cerr << "Usage: \"--target-denoised-error\" expects a relative error of the denoised frame >= 0 following it, e.g. --target-denoised-error 0.02 [--pass-spp K]." << endl;
                return -1;
            }
            toDenoisedError = true; ++i;
            continue;
        } else if (token == "--pass-spp") {
            char *end = nullptr;
            if (i + 1 < argc) passSpp = std::strtol(argv[i + 1], &end, 10);
            if (i + 1 >= argc || end == argv[i + 1] || *end != '\0' || passSpp <= 0 || passSpp > 0x7fffffffl) {
                cerr << "Usage: \"--pass-spp\" expects a positive number of samples per pixel and pass following it (with --target-error E)." << endl;
                return -1;
            }
            havePassSpp = true; ++i;
            continue;
        } else if (token == "--adaptive") {
            adaptive = true;
            continue;
        } else if (token == "--allocate") {
            allocate = true;
            continue;
        } else if (token == "--pilot-spp" || token == "--rounds") {
            const bool pilot = token == "--pilot-spp";
            char *end = nullptr;
            long v = -1;
            if (i + 1 < argc) v = std::strtol(argv[i + 1], &end, 10);
            if (i + 1 >= argc || end == argv[i + 1] || *end != '\0' || v < (pilot ? 2 : 1) || v > 0x7fffffffl) {
                cerr << "Usage: \"" << token << "\" expects " << (pilot ? "a number of samples per pixel >= 2 for the pilot" : "a number of rounds >= 1") << " following it (with --allocate)." << endl;
                return -1;
            }
            (pilot ? pilotSpp : rounds) = v;
            (pilot ? havePilotSpp : haveRounds) = true; ++i;
            continue;
        } else if (token == "--features") {
            features = true;
            continue;
        } else if (token == "--feature-spp") {
            char *end = nullptr;
            if (i + 1 < argc) featureSpp = std::strtol(argv[i + 1], &end, 10);
            if (i + 1 >= argc || end == argv[i + 1] || *end != '\0' || featureSpp <= 0 || featureSpp > 0x7fffffffl) {
                cerr << "Usage: \"--feature-spp\" expects a positive number of camera samples per pixel following it (with --features)." << endl;
                return -1;
            }
            haveFeatureSpp = true; ++i;
            continue;
        } else if (token == "--denoise") {
            denoise = true;
            continue;
        } else if (token == "--denoise-radius" || token == "--denoise-patch") {
            const bool radius = token == "--denoise-radius";
            const long lo = radius ? 1 : 0, hi = radius ? 8 : 2;
            char *end = nullptr;
            long v = -1;
            if (i + 1 < argc) v = std::strtol(argv[i + 1], &end, 10);
            if (i + 1 >= argc || end == argv[i + 1] || *end != '\0' || v < lo || v > hi) {
                cerr << "Usage: \"" << token << "\" expects a " << (radius ? "window radius 1 .. 8" : "patch radius 0 .. 2") << " following it (with --denoise)." << endl;
                return -1;
            }
            (radius ? denoiseRadius : denoisePatch) = v;
            (radius ? haveDenoiseRadius : haveDenoisePatch) = true; ++i;
            continue;
        } else if (token == "--aperture" || token == "--focus-distance") {
            const bool ap = token == "--aperture";
            char *end = nullptr;
            float v = -1.0f;
            if (i + 1 < argc) v = std::strtof(argv[i + 1], &end);
            if (i + 1 >= argc || end == argv[i + 1] || *end != '\0' || !std::isfinite(v) || (ap ? !(v >= 0.0f) : !(v > 0.0f))) {
                cerr << "Usage: \"" << token << "\" expects " << (ap ? "a lens radius >= 0 (0: the pinhole)" : "a focus distance > 0 (camera-space depth)") << " following it." << endl;
                return -1;
            }
            (ap ? aperture : focusDistance) = v;
            (ap ? haveAperture : haveFocusDistance) = true; ++i;
            continue;
        } else if (token == "--focus-pixel") {
            bool ok = i + 2 < argc;
            for (int k = 0; ok && k < 2; ++k) {
                char *end = nullptr;
                const long v = std::strtol(argv[i + 1 + k], &end, 10);
                ok = end != argv[i + 1 + k] && *end == '\0' && v >= 0 && v <= 0x7fffffffl;
                focusPixel[k] = v;
            }
            if (!ok) {
                cerr << "Usage: \"--focus-pixel\" expects the pixel X Y (two integers >= 0) whose surface the lens focuses on following it." << endl;
                return -1;
            }
            haveFocusPixel = true; i += 2;
            continue;
        } else if (token == "--split" || token == "--merge" || token == "--film-order") {
            if (i + 1 >= argc) {
                cerr << "\"" << token << "\" expects a value." << endl;
                return -1;
            }
            setenv(token == "--split" ? "NORI_SPLIT" : token == "--merge" ? "NORI_MERGE" : "NORI_FILM_ORDER", argv[++i], 1);
            continue;
        }
        if (endsWith(token, ".xml")) {
            sceneName = token;
            size_t slash = token.find_last_of('/');
            getFileResolver()->prepend(slash == std::string::npos ? std::string(".") : token.substr(0, slash));
        } else if (endsWith(token, ".exr")) {
            cerr << "The EXR viewer needs a display; this build has no GUI." << endl;
            return -1;
        } else {
            cerr << "Fatal error: unknown file \"" << token << "\", expected an extension of type .xml or .exr" << endl;
        }
    }
    if (allocate && adaptive) {
        cerr << "Usage: \"--allocate\" plans the samples from a pilot and does not go with --adaptive." << endl;
        return -1;
    }
    if (allocate && gpus > 1) {
        cerr << "Usage: \"--allocate\" renders on one device: moment frames over several GPUs are not supported (got --gpus " << gpus << ")." << endl;
        return -1;
    }
    if (allocate && !toError && !toDenoisedError) {
        cerr << "Usage: \"--allocate\" goes with --target-error E or --target-denoised-error E." << endl;
        return -1;
    }
    if ((havePilotSpp || haveRounds) && !allocate) {
        cerr << "Usage: \"" << (havePilotSpp ? "--pilot-spp" : "--rounds") << "\" goes with --allocate." << endl;
        return -1;
    }
    if (toDenoisedError && (denoise || toError || adaptive)) {
        cerr << "Usage: \"--target-denoised-error\" is a loop of its own and does not go with " << (denoise ? "--denoise" : toError ? "--target-error" : "--adaptive") << "." << endl;
        return -1;
    }
    if (toDenoisedError && gpus > 1) {
        cerr << "Usage: \"--target-denoised-error\" renders on one device: moment and feature frames over several GPUs are not supported (got --gpus " << gpus << ")." << endl;
        return -1;
    }
    if (havePassSpp && !toError && !toDenoisedError) {
        cerr << "Usage: \"--pass-spp\" goes with --target-error E." << endl;
        return -1;
    }
    if (adaptive && !toError) {
        cerr << "Usage: \"--adaptive\" goes with --target-error E." << endl;
        return -1;
    }
    if (toError && gpus > 1) {
        cerr << "\"--target-error\" renders on one device: moment frames over several GPUs are not supported (got --gpus " << gpus << ")." << endl;
        return -1;
    }
    if (haveFeatureSpp && !features && !denoise && !toDenoisedError) {
        cerr << "Usage: \"--feature-spp\" goes with --features (or --denoise)." << endl;
        return -1;
    }
    if ((haveDenoiseRadius || haveDenoisePatch) && !denoise && !toDenoisedError) {
        cerr << "Usage: \"" << (haveDenoiseRadius ? "--denoise-radius" : "--denoise-patch") << "\" goes with --denoise." << endl;
        return -1;
    }
    if (denoise && gpus > 1) {
        cerr << "Usage: \"--denoise\" renders on one device: moment and feature frames over several GPUs are not supported (got --gpus " << gpus << ")." << endl;
        return -1;
    }
    if (denoise && toError) {
        cerr << "Usage: \"--denoise\" renders the scene's sample count and does not go with --target-error." << endl;
        return -1;
    }
    if (features && gpus > 1) {
        cerr << "Usage: \"--features\" renders on one device: feature frames over several GPUs are not supported (got --gpus " << gpus << ")." << endl;
        return -1;
    }
    if (haveFocusPixel && haveFocusDistance) {
        cerr << "Usage: \"--focus-pixel\" sets the focus distance itself and does not go with --focus-distance." << endl;
        return -1;
    }
    if (sceneName.empty()) {
        cerr << "Please provide the path to a .xml (or .exr) file." << endl;
        return -1;
    }
    try {
        std::unique_ptr<NoriObject> root(loadFromXML(sceneName));
        if (root->getClassType() == NoriObject::EScene) {
            Scene *scene = static_cast<Scene *>(root.get());
            if (haveAperture || haveFocusDistance || haveFocusPixel) {
                const Camera *cam = scene->getCamera();
                float radius = haveAperture ? aperture : cam->getApertureRadius();
                float focus = haveFocusDistance ? focusDistance : cam->getFocusDistance();
                if (haveFocusPixel) {
                    /* the camera-space depth of what the PINHOLE ray through the pixel's centre hits: the twins of
                       PerspectiveCamera::sampleRay and Accel::rayIntersect, no kernel of its own */
                    if (focusPixel[0] >= cam->getOutputSize().x() || focusPixel[1] >= cam->getOutputSize().y())
                        throw NoriException("--focus-pixel %d %d lies outside the %d x %d frame", (int) focusPixel[0], (int) focusPixel[1], cam->getOutputSize().x(), cam->getOutputSize().y());
                    Device &dev = scene->device();
                    const float ps[2] = {(float) focusPixel[0] + 0.5f, (float) focusPixel[1] + 0.5f};
                    nori_ray r; nori_intersection its;
                    dev.check(nori_hip_sample_rays(dev.ctx(), ps, 1, &r), "nori_hip_sample_rays");
                    dev.check(nori_hip_intersect(dev.ctx(), &r, &its, 1, 0), "nori_hip_intersect");
                    if (its.mesh == NORI_NO_HIT)
                        throw NoriException("--focus-pixel %d %d: the camera ray through that pixel hits nothing to focus on", (int) focusPixel[0], (int) focusPixel[1]);
                    /* d.z in camera space: the ray's direction against the camera's axis, column 2 of cameraToWorld */
                    const float *m = scene->getDesc().camera.to_world;
                    const float az[3] = {m[2], m[6], m[10]};
                    const float dz = (az[0] * r.d[0] + az[1] * r.d[1] + az[2] * r.d[2]) / (az[0] * az[0] + az[1] * az[1] + az[2] * az[2]);
                    focus = its.t * dz;
                    if (!std::isfinite(focus) || !(focus > 0.0f))
                        throw NoriException("--focus-pixel %d %d: no usable depth (%f)", (int) focusPixel[0], (int) focusPixel[1], focus);
                    cout << "Focus distance " << focus << " (pixel " << focusPixel[0] << " " << focusPixel[1] << ")" << endl;
                }
                scene->setLens(radius, focus);
            }
            cout << "Rendering .. ";
            cout.flush();
            Timer timer;
            nori_render_stats st;
            uint32_t sppDone = 0;
            nori_error_summary summary;
            std::vector<float> errorMap;
            nori_adaptive_summary adaptiveSummary;
            std::vector<uint32_t> tileSpp;
            std::vector<float> denoised;
            nori_denoise_params dn = NORI_DENOISE_PARAMS_DEFAULT;
            dn.radius = (uint32_t) denoiseRadius; dn.patch = (uint32_t) denoisePatch;
            const uint32_t denoiseFeatureSpp = haveFeatureSpp ? (uint32_t) featureSpp
                                               : toDenoisedError ? (uint32_t) std::min<size_t>(scene->getSampler()->getSampleCount(), 16) : (uint32_t) scene->getSampler()->getSampleCount();
            nori_allocate_params ap;      /* --allocate: the pilot is no longer than the scene's samples unless --pilot-spp says so */
            ap.pilot_spp = havePilotSpp ? (uint32_t) pilotSpp : (uint32_t) std::max<size_t>(2, std::min<size_t>(scene->getSampler()->getSampleCount(), (size_t) pilotSpp));
            ap.max_rounds = (uint32_t) rounds; ap.target_tile_err = targetError; ap.headroom = 1.0f; ap.metric = toDenoisedError ? 1 : 0;
            const nori_allocate_params *apUsed = allocate ? &ap : nullptr;
            if (allocate && !toDenoisedError) adaptive = true;      /* the same files and the same report as --adaptive */
            std::unique_ptr<ImageBlock> result = toDenoisedError ? renderSceneAdaptiveDenoised(scene, targetError, (uint32_t) passSpp, dn, denoiseFeatureSpp, adaptiveSummary, denoised, errorMap, tileSpp, &st, apUsed)
                                                 : denoise ? renderSceneDenoised(scene, dn, denoiseFeatureSpp, denoised, &st)
                                                 : adaptive ? renderSceneAdaptive(scene, targetError, (uint32_t) passSpp, adaptiveSummary, errorMap, tileSpp, &st, apUsed)
                                                 : toError ? renderSceneToError(scene, targetError, (uint32_t) passSpp, sppDone, summary, errorMap, &st)
                                                         : renderScene(scene, &st);
            cout << "done. (took " << timer.elapsedString() << "; kernel " << timeString(st.kernel_ms, true) << ", "
                 << (double) (st.n_closest_rays + st.n_shadow_rays) / (st.kernel_ms * 1e3) << " Mrays/s)" << endl;
            std::unique_ptr<Bitmap> bitmap(result->toBitmap());
            std::string outputName = sceneName;
            size_t lastdot = outputName.find_last_of(".");
            if (lastdot != std::string::npos) outputName.erase(lastdot, std::string::npos);
            bitmap->saveEXR(outputName);
            bitmap->savePNG(outputName);
            if (adaptive || toDenoisedError) {
                const nori_error_summary &f = adaptiveSummary.frame;
                cout << (toDenoisedError ? "Denoised error: stopped after " : "Stopped after ") << adaptiveSummary.passes << (allocate ? " render calls (a pilot of " + std::to_string(ap.pilot_spp) + " samples per pixel, at most " + std::to_string(ap.max_rounds) + " rounds): " : " passes: ") << adaptiveSummary.spp_min << " to " << adaptiveSummary.spp_max << " samples per pixel, "
                     << adaptiveSummary.n_unconverged << " of " << adaptiveSummary.n_tiles << " tiles above the target " << targetError << (toDenoisedError ? "; mean predicted error of the denoised frame " : "; mean error ")
                     << f.sum_err / (double) std::max<uint64_t>(f.n_pixels, 1) << " (max " << f.max_err << ", " << f.n_above << " of " << f.n_pixels << " pixels above the target)" << endl;
                Bitmap errorBitmap(scene->getCamera()->getOutputSize()), sppBitmap(scene->getCamera()->getOutputSize());
                const int tilesX = ((int) errorBitmap.cols() + NORI_TILE_SIZE - 1) / NORI_TILE_SIZE;
                for (int y = 0; y < errorBitmap.rows(); ++y)
                    for (int x = 0; x < errorBitmap.cols(); ++x) {
                        errorBitmap.set(y, x, Color3f(errorMap[(size_t) y * errorBitmap.cols() + x]));
                        sppBitmap.set(y, x, Color3f((float) tileSpp[(size_t) (y / NORI_TILE_SIZE) * tilesX + x / NORI_TILE_SIZE]));
                    }
                errorBitmap.saveEXR(outputName + ".error");
                sppBitmap.saveEXR(outputName + ".spp");
            } else if (toError) {
                cout << "Stopped at " << sppDone << " samples per pixel: mean error " << summary.sum_err / (double) std::max<uint64_t>(summary.n_pixels, 1)
                     << " (target " << targetError << ", max " << summary.max_err << ", " << summary.n_above << " of " << summary.n_pixels << " pixels above the target)" << endl;
                Bitmap errorBitmap(scene->getCamera()->getOutputSize());
                for (int y = 0; y < errorBitmap.rows(); ++y)
                    for (int x = 0; x < errorBitmap.cols(); ++x)
                        errorBitmap.set(y, x, Color3f(errorMap[(size_t) y * errorBitmap.cols() + x]));
                errorBitmap.saveEXR(outputName + ".error");
            }
            if (denoise || toDenoisedError) {
                Bitmap db(scene->getCamera()->getOutputSize());
                for (int y = 0; y < db.rows(); ++y)
                    for (int x = 0; x < db.cols(); ++x) {
                        const float *p = &denoised[((size_t) y * db.cols() + x) * 3];
                        db.set(y, x, Color3f(p[0], p[1], p[2]));
                    }
                db.saveEXR(outputName + ".denoised");
                cout << "Denoised (window radius " << denoiseRadius << ", patch radius " << denoisePatch << ", features of " << denoiseFeatureSpp
                     << " samples per pixel) to " << outputName << ".denoised.exr" << endl;
            }
            if (features) {
                const uint32_t spp = haveFeatureSpp ? (uint32_t) featureSpp : (uint32_t) std::min<size_t>(scene->getSampler()->getSampleCount(), 16);
                std::vector<float> fa, fn, fd;
                int border = 0;
                nori_render_stats fst;
                Timer ftimer;
                renderSceneFeatures(scene, spp, fa, fn, fd, border, &fst);
                cout << "Feature frames (albedo, normal, depth) of " << spp << " samples per pixel: took " << ftimer.elapsedString() << "; kernel "
                     << timeString(fst.kernel_ms, true) << ", " << fst.n_closest_rays << " rays" << endl;
                const Vector2i size = scene->getCamera()->getOutputSize();
                Bitmap ba(size), bn(size), bd(size);
                const int cols = size.x() + 2 * border;
                /* the decode of include/nori_hip.h: each quotient 0 where its divisor is <= 0 */
                auto quot = [](float a, float b) { return b > 0.0f ? a / b : 0.0f; };
                for (int y = 0; y < size.y(); ++y)
                    for (int x = 0; x < size.x(); ++x) {
                        const size_t i = ((size_t) (y + border) * cols + (x + border)) * 4;
                        ba.set(y, x, Color3f(quot(fa[i], fa[i + 3]), quot(fa[i + 1], fa[i + 3]), quot(fa[i + 2], fa[i + 3])));
                        if (fn[i + 3] > 0.0f) bn.set(y, x, Color3f(2.0f * (fn[i] / fn[i + 3]) - 1.0f, 2.0f * (fn[i + 1] / fn[i + 3]) - 1.0f, 2.0f * (fn[i + 2] / fn[i + 3]) - 1.0f));
                        else bn.set(y, x, Color3f(0.0f));
                        bd.set(y, x, Color3f(quot(fd[i], fd[i + 2]), quot(fd[i + 2], fd[i + 3]), quot(fd[i + 1], fd[i + 2])));
                    }
                ba.saveEXR(outputName + ".albedo");
                bn.saveEXR(outputName + ".normal");
                bd.saveEXR(outputName + ".depth");
            }
        }
    } catch (const std::exception &e) {
        cerr << e.what() << endl;
        return -1;
    }
    return 0;
}
