// vxpt_offline -- the offline renderer executable over the vxpt C ABI.
//
// Mirrors the reference's mainOffline.cpp (flags :57-133, set-up :140-251, frame loop :273-408,
// canonical gate :423-498) and OfflineBackend::renderFrame / writeAllBatchedFrames
// (OfflineBackend.cpp:46-184).  Host code only: every GPU operation goes through include/vxpt.h.
//
// Same flags and outputs as the reference: saved frames are the 1-indexed {1, 4, 16, 64} written
// as <prefix>_%04d.png with the 0-indexed frame number, the canonical gate compares frame
// totalFrames-1 and writes <prefix>_diff.png.  Additions: --spp (samples per pixel per frame,
// the reference traces 1), --chunks X Y Z (world size, default the reference's 2 1 2), --device,
// --data (the data directory), --perf-report (the run summary file; default <data>/perf/
// performance_report.txt, the reference's data/perf/performance_report.txt), and a per-frame CSV
// <prefix>_frames.csv of the library's timings; --render-scale S traces and post-processes at S times
// the output size and brings the frame up to it with vxpt_upscale (--upscale, --sharpness) before it
// is saved: the reference's interactive back end does the same (Backend::dynamicResolution), its
// offline one does not; --render-size-schedule and --dynamic-resolution move the render size between frames
// (vxpt_set_render_size, the histories carried over) with every saved frame scaled up.  --time-of-day, --sun-axis-angle, --sun-axis-rotate and --sky-build set the sky
// (the reference reads it from its settings; here the defaults are its values 0.25, 45, 0).
// The scripted voxel-edit sequences (--test-sequence, --test-remove20, --test-remove-circle) follow
// the reference's timing: a click set after frame N is picked at frame N+1 against the world as
// edited so far (VoxelEngine::update, VoxelEngine.cu:906-975) and the geometry changes at frame
// N+2 (OptixRenderer::update rebuilds the chunk's acceleration structure a frame later,
// OptixRenderer.cpp:846-925), the frame whose ReSTIR temporal visibility sees no previous scene.
#include "../../include/vxpt.h"

#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <ctime>
#include <filesystem>
#include <fstream>
#include <future>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>
#include <iomanip>

namespace {

struct Options {
    int width = 3840, height = 2160;
    std::string outputPrefix = "offline_render";
    std::string sceneFile = "data/scene/scene_export.yaml";
    bool testCanonical = false, updateCanonical = false;
    std::string canonicalImagePath = "../../data/canonical/canonical_render.png";
    std::string runComment = "default run";
    int totalFrames = 64;
    std::vector<int> savedFrames = {1, 4, 16, 64};
    int spp = 1;
    int chunks[3] = {2, 1, 2};
    int device = 0;
    std::string dataDir = "data";
    std::string assetsDir;  // root of the instanced meshes' OBJ files (empty: the data directory)
    std::string perfReport;
    bool testSequence = false, removal20 = false, removalCircle = false;
    bool textures = true;
    // block-compressed textures (vxpt_load_textures_bc): blocks decoded in the sampler, or expanded to RGBA8
    bool bcTextures = false, expandTextures = false;
    int bcEncoder = -1;  // --bc-encoder: 0 fast, 1 search (VXPT_TEX_ENCODE_SEARCH); -1: not given
    std::string textureCache;  // the reference's cache directory (<name>_lod_<n>.bin); empty: none
    // render scale: trace at renderWidth x renderHeight, save width x height (1: no upscale at all)
    float renderScale = 1.0f, sharpness = 1.0f;
    int upscaleMode = VXPT_UPSCALE_EASU_SHARPEN;
    int renderWidth = 0, renderHeight = 0;
    // dynamic resolution (vxpt_set_render_size): the size set before frame F (0-based) of a schedule, or the
    // reference's controller on each frame's measured time (targetFps 0: the settings file's)
    struct SizeAt { int frame, w, h; };
    std::vector<SizeAt> sizeSchedule;
    bool dynamicResolution = false;
    float targetFps = 0.0f;
    // the sky: time of day (a T0:T1 range moves it linearly over the frames and sets it before each),
    // the sun's axis, and where the tables are built (-1: device for a range, host otherwise)
    float tod0 = 0.25f, tod1 = 0.25f, sunAxisAngle = 45.0f, sunAxisRotate = 0.0f;
    bool todRange = false;
    int skyBuild = -1;
    int worldBuild = VXPT_WORLD_BUILD_HOST;  // --world-build
    int instanceBuild = VXPT_INSTANCE_BUILD_HOST;  // --instance-build
    // --load-world: the world (and, unless --scene is given, the camera) from a saved scene instead of the terrain
    std::string worldYaml, worldChunks;
    bool sceneGiven = false;
    // --terrain-origin / --terrain-seed: the terrain through vxpt_generate_terrain_ex
    bool terrainEx = false;
    int terrainOrigin[3] = {0, 0, 0};
    unsigned terrainSeed = 124;
};

const char *upscale_name(int mode) {
    return mode == VXPT_UPSCALE_BICUBIC ? "bicubic" : mode == VXPT_UPSCALE_EASU ? "easu" : "easu-sharp";
}

void usage(const char *argv0) {
    std::cout << "Offline Voxel Path Tracer (MI355X)\n"
              << "Usage: " << argv0 << " [options]\n"
              << "Options:\n"
              << "  --width <int>          Output width (default: 3840)\n"
              << "  --height <int>         Output height (default: 2160)\n"
              << "  --output <string>      Output filename prefix (default: offline_render)\n"
              << "  --scene <file>         Scene configuration YAML file (camera)\n"
              << "  --test-canonical       Compare output with canonical image\n"
              << "  --update-canonical     Update the canonical reference image\n"
              << "  --canonical-image <p>  Path to canonical image (default: ../../data/canonical/canonical_render.png)\n"
              << "  --comment <text>       Comment for performance report (default: default run)\n"
              << "  --test-sequence        Enable scripted block placement test sequence\n"
              << "  --test-remove20        Enable scripted removal test (20 deletions)\n"
              << "  --test-remove-circle   Enable circular removal test (8 directions, 5 deletions each)\n"
              << "  --world-build <m>      host (default) or device: where the walk's tables are built and edited\n"
              << "  --instance-build <m>   host (default) or device: where an instanced-block edit refreshes the TLAS\n"
              << "                         and the light tables\n"
              << "  --load-world <yaml> <dir>  The world from a saved scene (vxpt_save_world: scene yaml and chunk\n"
              << "                         directory) instead of the generated terrain; its camera too unless\n"
              << "                         --scene is given\n"
              << "  --terrain-origin <x,y,z>  Cells added to the terrain window's x, y, z (default: 0,0,0; y must be 0)\n"
              << "  --terrain-seed <n>     Seed of the terrain's noise (default: 124).  With either flag the terrain is\n"
              << "                         generated on the device when --world-build is device\n"
              << "  --frames <int>         Number of frames to render (default: 64, use 1 for single frame)\n"
              << "  --spp <int>            Samples per pixel per frame (default: 1)\n"
              << "  --chunks <x> <y> <z>   World size in 32^3 chunks (default: 2 1 2)\n"
              << "  --device <int>         HIP device (default: 0)\n"
              << "  --data <dir>           Data directory: settings/, assets/, tables/ (default: data)\n"
              << "  --models <dir>         Root of the instanced meshes' OBJ files (<dir>/models/*.obj; default: the data directory)\n"
              << "  --perf-report <file>   Performance report the run summary is appended to\n"
              << "                         (default: <data>/perf/performance_report.txt)\n"
              << "  --no-textures          Untextured materials (textures load from <data>/textures when present)\n"
              << "  --bc-textures          Keep the textures as BC7 / BC5 / BC4 blocks, decoded in the sampler\n"
              << "  --texture-cache <dir>  Read <name>_lod_<n>.bin block files from <dir> (the reference's texture\n"
              << "                         cache) and write the levels encoded here; implies --bc-textures\n"
              << "  --expand-textures      With --bc-textures: decode the blocks to RGBA8 texels on the host\n"
              << "  --bc-encoder <e>       With --bc-textures: fast (default; the host encoder) or search (the search\n"
              << "                         encoder on the device) for the levels that have no cache file\n"
              << "  --render-scale <s>     Trace at s times the output size, 0.25 <= s <= 1 (default: 1); each side is\n"
              << "                         rounded to a multiple of 8 (at least 8) and the frame is scaled up to\n"
              << "                         --width x --height before it is saved.  The post-process runs at the\n"
              << "                         render size, so its crosshair is scaled up with the frame.  1 renders\n"
              << "                         at the output size as before\n"
              << "  --upscale <filter>     bicubic | easu | easu-sharp (default: easu-sharp): Catmull-Rom, the\n"
              << "                         edge-adaptive upsampler, or the upsampler and the sharpener\n"
              << "  --sharpness <f>        Strength of easu-sharp's sharpener, 0 <= f <= 1 (default: 1)\n"
              << "  --render-size-schedule F:WxH[,F:WxH...]\n"
              << "                         Set the render size to W x H before frame F (counted from 0), at most the\n"
              << "                         size the run starts at; the histories are carried over.  Every saved frame\n"
              << "                         is scaled up to --width x --height with the --upscale filter\n"
              << "  --dynamic-resolution   Set the render size after every frame from its measured time, by the\n"
              << "                         reference's rule (16:9 sizes, widths in multiples of 16 between the\n"
              << "                         settings' minRenderWidth and the starting width); not deterministic\n"
              << "  --target-fps <n>       The controller's target (default: the settings' targetFPS)\n"
              << "  --time-of-day <t>      Time of day of the sky (default: 0.25), or T0:T1: the time moves linearly\n"
              << "                         from T0 at the first frame to T1 at the last, the sky is rebuilt before\n"
              << "                         each frame, and every frame is saved\n"
              << "  --sun-axis-angle <deg> Tilt of the sun's axis (default: 45)\n"
              << "  --sun-axis-rotate <deg> Rotation of the sun's axis (default: 0)\n"
              << "  --sky-build <where>    host | device: Vose tables built on the host (waits for the GPU), or\n"
              << "                         the parallel construction on the GPU (default: device for a T0:T1\n"
              << "                         range, host otherwise)\n"
              << "  --help, -h             Show this help message\n";
}

// returns 1 = run, 0 = exit 0 (help), -1 = exit 2 (bad args)
int parse(int argc, char **argv, Options &o) {
    for (int i = 1; i < argc; i++) {
        const std::string a = argv[i];
        // mainOffline.cpp:57-133 reads a flag's value only when one follows (`&& i + 1 < argc`)
        // and skips anything it does not know: a trailing valueless flag and unknown
        // arguments are ignored here too (with a note on stderr), so reference scripts run as-is
        auto next = [&](const char *what) -> const char * {
            if (i + 1 >= argc) {
                std::cerr << "note: " << what << " without a value ignored\n";
                return nullptr;
            }
            return argv[++i];
        };
        const char *v = nullptr;
        if (a == "--width") { if ((v = next("--width"))) { o.width = std::atoi(v); } }
        else if (a == "--height") { if ((v = next("--height"))) { o.height = std::atoi(v); } }
        else if (a == "--output") { if ((v = next("--output"))) { o.outputPrefix = v; } }
        else if (a == "--scene") { if ((v = next("--scene"))) { o.sceneFile = v; o.sceneGiven = true; } }
        else if (a == "--test-canonical" || a == "--test") o.testCanonical = true;
        else if (a == "--update-canonical") o.updateCanonical = true;
        else if (a == "--canonical-image") { if ((v = next("--canonical-image"))) { o.canonicalImagePath = v; } }
        else if (a == "--comment") { if ((v = next("--comment"))) { o.runComment = v; } }
        else if (a == "--frames") {
            if ((v = next("--frames"))) {
                o.totalFrames = std::atoi(v);
                if (o.totalFrames == 1) o.savedFrames = {1};  // mainOffline.cpp:108-111
            }
        }
        else if (a == "--spp") { if ((v = next("--spp"))) { o.spp = std::atoi(v); } }
        else if (a == "--chunks") {
            for (int k = 0; k < 3; k++) {
                if (!(v = next("--chunks"))) return -1;  // an extension flag: all three values required
                o.chunks[k] = std::atoi(v);
            }
        }
        else if (a == "--device") { if ((v = next("--device"))) { o.device = std::atoi(v); } }
        else if (a == "--data") { if ((v = next("--data"))) { o.dataDir = v; } }
        else if (a == "--models") { if ((v = next("--models"))) { o.assetsDir = v; } }
        else if (a == "--perf-report") { if ((v = next("--perf-report"))) { o.perfReport = v; } }
        else if (a == "--no-textures") o.textures = false;
        else if (a == "--bc-textures") o.bcTextures = true;
        else if (a == "--expand-textures") o.bcTextures = o.expandTextures = true;
        else if (a == "--texture-cache") { if ((v = next("--texture-cache"))) { o.textureCache = v; o.bcTextures = true; } }
        else if (a == "--bc-encoder") {
            if ((v = next("--bc-encoder"))) {
                const std::string m = v;
                if (m == "fast") o.bcEncoder = 0;
                else if (m == "search") o.bcEncoder = 1;
                else {
                    std::cerr << "--bc-encoder takes fast or search\n";
                    return -1;
                }
            }
        }
        else if (a == "--render-scale") { if ((v = next("--render-scale"))) { o.renderScale = (float)std::atof(v); } }
        else if (a == "--render-size-schedule") {
            if ((v = next("--render-size-schedule"))) {
                std::stringstream ss(v);
                std::string item;
                while (std::getline(ss, item, ',')) {
                    Options::SizeAt e{};
                    char tail = 0;
                    if (std::sscanf(item.c_str(), "%d:%dx%d%c", &e.frame, &e.w, &e.h, &tail) != 3 || e.frame < 0 || e.w < 1 ||
                        e.h < 1) {
                        std::cerr << "--render-size-schedule takes F:WxH[,F:WxH...]\n";
                        return -1;
                    }
                    o.sizeSchedule.push_back(e);
                }
            }
        }
        else if (a == "--dynamic-resolution") o.dynamicResolution = true;
        else if (a == "--target-fps") { if ((v = next("--target-fps"))) { o.targetFps = (float)std::atof(v); } }
        else if (a == "--sharpness") { if ((v = next("--sharpness"))) { o.sharpness = (float)std::atof(v); } }
        else if (a == "--upscale") {
            if ((v = next("--upscale"))) {
                const std::string m = v;
                if (m == "bicubic") o.upscaleMode = VXPT_UPSCALE_BICUBIC;
                else if (m == "easu") o.upscaleMode = VXPT_UPSCALE_EASU;
                else if (m == "easu-sharp") o.upscaleMode = VXPT_UPSCALE_EASU_SHARPEN;
                else {
                    std::cerr << "--upscale takes bicubic, easu or easu-sharp\n";
                    return -1;
                }
            }
        }
        else if (a == "--time-of-day") {
            if ((v = next("--time-of-day"))) {
                const std::string t = v;
                const size_t colon = t.find(':');
                o.tod0 = o.tod1 = (float)std::atof(t.substr(0, colon).c_str());
                o.todRange = colon != std::string::npos;
                if (o.todRange) o.tod1 = (float)std::atof(t.substr(colon + 1).c_str());
            }
        }
        else if (a == "--sun-axis-angle") { if ((v = next("--sun-axis-angle"))) { o.sunAxisAngle = (float)std::atof(v); } }
        else if (a == "--sun-axis-rotate") { if ((v = next("--sun-axis-rotate"))) { o.sunAxisRotate = (float)std::atof(v); } }
        else if (a == "--sky-build") {
            if ((v = next("--sky-build"))) {
                const std::string m = v;
                if (m == "host") o.skyBuild = 0;
                else if (m == "device") o.skyBuild = 1;
                else {
                    std::cerr << "--sky-build takes host or device\n";
                    return -1;
                }
            }
        }
        else if (a == "--world-build") {
            if ((v = next("--world-build"))) {
                const std::string m = v;
                if (m == "host") o.worldBuild = VXPT_WORLD_BUILD_HOST;
                else if (m == "device") o.worldBuild = VXPT_WORLD_BUILD_DEVICE;
                else {
                    std::cerr << "--world-build takes host or device\n";
                    return -1;
                }
            }
        }
        else if (a == "--instance-build") {
            if ((v = next("--instance-build"))) {
                const std::string m = v;
                if (m == "host") o.instanceBuild = VXPT_INSTANCE_BUILD_HOST;
                else if (m == "device") o.instanceBuild = VXPT_INSTANCE_BUILD_DEVICE;
                else {
                    std::cerr << "--instance-build takes host or device\n";
                    return -1;
                }
            }
        }
        else if (a == "--load-world") {
            if (!(v = next("--load-world"))) return -1;  // an extension flag: both values required
            o.worldYaml = v;
            if (!(v = next("--load-world"))) return -1;
            o.worldChunks = v;
        }
        else if (a == "--terrain-origin") {
            if (!(v = next("--terrain-origin"))) return -1;
            char tail = 0;
            if (std::sscanf(v, "%d,%d,%d%c", &o.terrainOrigin[0], &o.terrainOrigin[1], &o.terrainOrigin[2], &tail) != 3) {
                std::cerr << "--terrain-origin takes X,Y,Z\n";
                return -1;
            }
            o.terrainEx = true;
        }
        else if (a == "--terrain-seed") {
            if (!(v = next("--terrain-seed"))) return -1;
            char *end = nullptr;
            o.terrainSeed = (unsigned)std::strtoul(v, &end, 10);
            if (end == v || *end) {
                std::cerr << "--terrain-seed takes an unsigned integer\n";
                return -1;
            }
            o.terrainEx = true;
        }
        else if (a == "--test-sequence") o.testSequence = true;
        else if (a == "--test-remove20") o.removal20 = true;
        else if (a == "--test-remove-circle") o.removalCircle = true;
        else if (a == "--help" || a == "-h") { usage(argv[0]); return 0; }
        else std::cerr << "note: unknown option " << a << " ignored\n";
    }
    if (o.width <= 0 || o.height <= 0) {
        std::cerr << "width and height must be positive\n";
        return -1;
    }
    if (o.totalFrames <= 0 || o.spp <= 0 || o.chunks[0] <= 0 || o.chunks[1] <= 0 || o.chunks[2] <= 0) {
        std::cerr << "frames, spp and chunks must be positive\n";
        return -1;
    }
    if (!(o.renderScale >= 0.25f && o.renderScale <= 1.0f) || !(o.sharpness >= 0.0f && o.sharpness <= 1.0f)) {
        std::cerr << "render-scale must lie in [0.25, 1] and sharpness in [0, 1]\n";
        return -1;
    }
    if (o.bcEncoder >= 0 && !o.bcTextures) {
        std::cerr << "--bc-encoder needs --bc-textures\n";
        return -1;
    }
    if (o.skyBuild < 0) o.skyBuild = o.todRange ? 1 : 0;
    if (o.todRange) {  // a day cycle is an animation: every frame is saved
        o.savedFrames.clear();
        for (int f = 1; f <= o.totalFrames; f++) o.savedFrames.push_back(f);
    }
    o.renderWidth = o.width;
    o.renderHeight = o.height;
    if (o.renderScale < 1.0f) {
        if (o.width < 8 || o.height < 8) {
            std::cerr << "render-scale below 1 needs an output of at least 8x8\n";
            return -1;
        }
        // a multiple of 8, at least 8 and no larger than the output
        auto side = [&](int out) {
            const int r = (int)std::lround((double)out * o.renderScale / 8.0) * 8;
            return std::min(std::max(r, 8), out / 8 * 8);
        };
        o.renderWidth = side(o.width);
        o.renderHeight = side(o.height);
    }
    for (const auto &e : o.sizeSchedule)
        if (e.w > o.renderWidth || e.h > o.renderHeight) {
            std::cerr << "--render-size-schedule: " << e.w << "x" << e.h << " is larger than the starting size "
                      << o.renderWidth << "x" << o.renderHeight << "\n";
            return -1;
        }
    if (o.dynamicResolution && !o.sizeSchedule.empty()) {
        std::cerr << "--dynamic-resolution and --render-size-schedule exclude each other\n";
        return -1;
    }
    if (o.targetFps != 0.0f && (!o.dynamicResolution || !(o.targetFps > 2.0f))) {
        std::cerr << "--target-fps needs --dynamic-resolution and a value above 2\n";
        return -1;
    }
    if (o.perfReport.empty()) o.perfReport = o.dataDir + "/perf/performance_report.txt";
    return 1;
}

std::string frame_path(const std::string &prefix, int frame0) {
    std::ostringstream s;
    s << prefix << "_" << std::setfill('0') << std::setw(4) << frame0 << ".png";
    return s.str();
}

struct BatchedFrame {
    std::vector<float> rgba;
    std::string path;
};

struct FrameRecord {  // PerformanceTracker's per-frame row, from the library's HIP-event timings
    int frame;
    std::string comment;
    vxpt_timing t;
    double postMs, wallMs;
    float dtMs;
    double updateMs;  // the frame's voxel-engine update on the host (clicks, picks, block edits)
};

// PerformanceTracker's timestamp format (PerformanceTracker.h: "%Y-%m-%d %H:%M:%S.mmm", local time)
std::string timestamp_now() {
    const auto now = std::chrono::system_clock::now();
    const std::time_t tt = std::chrono::system_clock::to_time_t(now);
    const long ms = (long)(std::chrono::duration_cast<std::chrono::milliseconds>(now.time_since_epoch()).count() % 1000);
    std::tm tmv{};
    localtime_r(&tt, &tmv);
    std::ostringstream ss;
    ss << std::put_time(&tmv, "%Y-%m-%d %H:%M:%S") << '.' << std::setfill('0') << std::setw(3) << ms;
    return ss.str();
}

// PerformanceTracker::saveReport (PerformanceTracker.h:98-183): one run-summary line appended to the
// report, the header first when the file is new; columns are per-frame averages in ms.  Here
// PathTrace and Denoiser are the library's HIP-event times (the reference's are CPU launch times),
// ScenePrep is 0 (the sky is built before the loop, or per frame by --time-of-day T0:T1), RendererUpd the host's
// voxel-engine update.
bool append_run_summary(const std::string &path, const std::string &stamp, int w, int h,
                        const std::vector<FrameRecord> &perf, const std::string &comment) {
    if (perf.empty()) return true;
    const std::filesystem::path fp(path);
    std::error_code ec;
    if (fp.has_parent_path()) std::filesystem::create_directories(fp.parent_path(), ec);
    std::ofstream f(path, std::ios::app);
    if (!f) return false;
    f.seekp(0, std::ios::end);
    if (f.tellp() == 0)
        f << "# Performance Report - Real-time Path Tracing Voxel Renderer (Run Summary)\n"
          << "# Format: Timestamp         | Frames | Resolution | WholeFrame | StdDev | ScenePrep | RendererUpd | "
             "PathTrace | Denoiser | PostProc | Comment\n"
          << "# ==========================================================================================="
             "====================================\n";
    double whole = 0, upd = 0, trace = 0, den = 0, post = 0;
    for (const auto &r : perf) {
        whole += r.wallMs; upd += r.updateMs; trace += r.t.trace_ms; den += r.t.denoise_ms; post += r.postMs;
    }
    const double n = (double)perf.size();
    whole /= n; upd /= n; trace /= n; den /= n; post /= n;
    double var = 0;
    for (const auto &r : perf) var += (r.wallMs - whole) * (r.wallMs - whole);
    const double sd = std::sqrt(var / n);
    f << std::fixed << std::setprecision(2);
    f << std::setw(19) << std::left << stamp << " | ";
    f << std::setw(6) << std::right << perf.size() << " | ";
    f << std::setw(10) << std::left << (std::to_string(w) + "x" + std::to_string(h)) << " | ";
    f << std::setw(10) << std::right << whole << " | ";
    f << std::setw(6) << std::right << sd << " | ";
    f << std::setw(9) << std::right << 0.0 << " | ";
    f << std::setw(11) << std::right << upd << " | ";
    f << std::setw(9) << std::right << trace << " | ";
    f << std::setw(8) << std::right << den << " | ";
    f << std::setw(8) << std::right << post << " | ";
    f << comment << std::endl;
    return (bool)f;
}

void print_diff(const vxpt_image_diff_result &r) {  // ImageDiffResult::print (ImageDiff.cpp)
    std::cout << "=== Image Comparison Results ===\n"
              << "Total pixels: " << r.total_pixels << "\n"
              << "Different pixels: " << r.different_pixels << " (" << std::fixed << std::setprecision(2)
              << r.pixel_difference_ratio * 100.0f << "%)\n"
              << std::setprecision(4) << "RMSE: " << r.rmse << "\n"
              << "SSIM: " << r.ssim << "\n"
              << "Assessment: "
              << (r.is_identical ? "IDENTICAL" : r.is_very_close ? "VERY CLOSE" : r.is_close ? "CLOSE" : "DIFFERENT")
              << "\n";
    std::cout.unsetf(std::ios::floatfield);
}

}  // namespace

int main(int argc, char **argv) {
    Options o;
    const int pr = parse(argc, argv, o);
    if (pr <= 0) return pr == 0 ? 0 : 2;

    std::cout << "=== Offline Voxel Path Tracer ===\n"
              << "Resolution: " << o.width << "x" << o.height << "\n"
              << (o.renderScale < 1.0f ? "Render scale: " + std::to_string(o.renderScale) + " (" +
                                             std::to_string(o.renderWidth) + "x" + std::to_string(o.renderHeight) +
                                             " traced, " + upscale_name(o.upscaleMode) + " to the resolution)\n"
                                       : std::string())
              << (o.dynamicResolution ? "Dynamic resolution: on, from each frame's measured time\n" : std::string())
              << "Frames to render: " << o.totalFrames << " at " << o.spp << " spp\n"
              << "Output prefix: " << o.outputPrefix << std::endl;
    for (const auto &e : o.sizeSchedule)
        std::cout << "Render size schedule: " << e.w << "x" << e.h << " from frame " << e.frame << std::endl;

    vxpt_config cfg{};
    cfg.width = o.renderWidth;
    cfg.height = o.renderHeight;
    cfg.device = o.device;
    cfg.total_bounce_limit = 3;    // RayGen.cu:146
    cfg.diffuse_bounce_limit = 1;  // RayGen.cu:147
    cfg.data_dir = o.dataDir.c_str();
    vxpt_ctx *ctx = nullptr;
    if (vxpt_create(&cfg, &ctx) != VXPT_OK) {
        std::cerr << "Error: vxpt_create failed: " << vxpt_last_error(ctx) << std::endl;
        vxpt_destroy(ctx);
        return 1;
    }
    auto last = std::chrono::steady_clock::now();  // OfflineBackend::init starts m_timer (OfflineBackend.cpp:43)
    auto fail = [&](const char *what) {
        std::cerr << "Error: " << what << ": " << vxpt_last_error(ctx) << std::endl;
        vxpt_destroy(ctx);
        return 1;
    };

    // mainOffline.cpp:140-198: settings, assets, the voxel world
    if (vxpt_load_settings(ctx) != VXPT_OK) return fail("loading settings");
    if (o.textures) {  // TextureManager::initWithMaterialPaths: every material texture found is used
        int nTex = 0;
        if (o.bcTextures) {
            int nCached = 0;
            const int flags = (o.textureCache.empty() ? 0 : VXPT_TEX_WRITE_CACHE) | (o.expandTextures ? VXPT_TEX_EXPAND : 0) |
                              (o.bcEncoder == 1 ? VXPT_TEX_ENCODE_SEARCH : 0);
            if (vxpt_load_textures_bc(ctx, nullptr, o.textureCache.empty() ? nullptr : o.textureCache.c_str(), flags, &nTex,
                                      &nCached) != VXPT_OK)
                return fail("loading textures");
            std::cout << "Block-compressed textures" << (o.expandTextures ? " (expanded to RGBA8)" : "") << ": " << nCached
                      << " levels from the cache" << std::endl;
        } else if (vxpt_load_textures(ctx, nullptr, &nTex) != VXPT_OK) return fail("loading textures");
        std::cout << "Textures loaded: " << nTex << (nTex ? "" : " (untextured materials)") << std::endl;
    }
    if (vxpt_set_world_build(ctx, o.worldBuild) != VXPT_OK) return fail("setting the world build mode");
    if (o.instanceBuild != VXPT_INSTANCE_BUILD_HOST && vxpt_set_instance_build(ctx, o.instanceBuild) != VXPT_OK)
        return fail("setting the instance build mode");
    vxpt_camera worldCam{};
    if (!o.worldYaml.empty()) {
        if (vxpt_load_world(ctx, o.worldYaml.c_str(), o.worldChunks.c_str(), &worldCam) != VXPT_OK)
            return fail("loading the world");
        std::cout << "World loaded: " << o.worldYaml << std::endl;
    } else if (o.terrainEx) {
        const vxpt_terrain_desc td{{o.chunks[0], o.chunks[1], o.chunks[2]}, 32.0f, 32.0f * o.chunks[0], 0,
                                   {o.terrainOrigin[0], o.terrainOrigin[1], o.terrainOrigin[2]}, o.terrainSeed};
        if (vxpt_generate_terrain_ex(ctx, &td) != VXPT_OK) return fail("generating terrain");
    } else if (vxpt_generate_terrain(ctx, o.chunks[0], o.chunks[1], o.chunks[2], 32.0f, 32.0f * o.chunks[0], 0) != VXPT_OK)
        return fail("generating terrain");
    // VoxelEngine::init (VoxelEngine.cu:809-816): the instanced meshes, their instances in the world and
    // the light table (a full light update); block types whose OBJ file is missing stay empty
    {
        int nModels = 0;
        const int rc = vxpt_load_models(ctx, o.assetsDir.empty() ? nullptr : o.assetsDir.c_str(), &nModels);
        if (rc == VXPT_ERR_IO)  // a data directory without the asset yaml files: no instanced blocks
            std::cout << "Instanced meshes not loaded: " << vxpt_last_error(ctx) << std::endl;
        else if (rc != VXPT_OK)
            return fail("loading the instanced meshes");
        else
            std::cout << "Instanced meshes loaded: " << nModels << std::endl;
    }

    // :200-251: camera from the scene file (defaults when it is absent), history camera = camera
    vxpt_camera cam{};
    const bool haveScene = !o.sceneFile.empty() && std::filesystem::exists(o.sceneFile);
    if (!haveScene && !o.sceneFile.empty())
        std::cout << "Scene file not found: " << o.sceneFile << ", using defaults" << std::endl;
    if (vxpt_load_scene_camera(ctx, haveScene ? o.sceneFile.c_str() : nullptr, &cam) != VXPT_OK)
        return fail("loading the scene camera");
    if (!o.worldYaml.empty() && !o.sceneGiven) cam = worldCam;
    if (vxpt_set_camera(ctx, &cam, &cam) != VXPT_OK) return fail("setting the camera");
    auto set_sky = [&](float tod) {
        return (o.skyBuild ? vxpt_set_sky_device : vxpt_set_sky)(ctx, tod, o.sunAxisAngle, o.sunAxisRotate, 1.0f);
    };
    if (set_sky(o.tod0) != VXPT_OK) return fail("building the sky");
    std::cout << "Camera setup - Position: (" << cam.pos[0] << ", " << cam.pos[1] << ", " << cam.pos[2] << ")\n"
              << "Camera setup - Direction: (" << cam.dir[0] << ", " << cam.dir[1] << ", " << cam.dir[2] << ")\n"
              << "Camera setup - FOV: " << cam.fov_deg << " degrees\n"
              << "Camera movement: DISABLED (static camera)\nStarting rendering..." << std::endl;

    vxpt_denoise_params dp{};
    vxpt_post_params pp{};
    if (vxpt_get_post_params(ctx, &pp) != VXPT_OK) return fail("reading post-process settings");
    if (vxpt_get_denoise_params(ctx, &dp) != VXPT_OK) return fail("reading denoise settings");

    // scripted clicks (mainOffline.cpp:43-50, 166-188, 281-395; VoxelEngine.cu:206-217, 906-945)
    constexpr int kRemovals20 = 20, kDirections = 8, kPerDirection = 5, kCircleRemovals = kDirections * kPerDirection;
    constexpr float kPi = 3.14159265358979323846f, kPiOver180 = kPi / 180.0f, kTwoPi = 2.0f * kPi;
    constexpr float kYawAmp = 12.0f * kPiOver180, kPitchAmp = 6.0f * kPiOver180;
    std::vector<int> clickSequence;  // empty: the default {16, 0, 16} cycle
    if (o.removalCircle) clickSequence.assign(kCircleRemovals, 0);
    else if (o.removal20) clickSequence.assign(kRemovals20, 0);
    size_t clickIndex = 0, defaultIndex = 0;
    bool clickPending = false, editPending = false;
    int edit[4] = {0, 0, 0, 0};
    int removals = 0, circleDone = 0, lastDirection = -1;
    bool circleRestored = false;
    float camInfo[32];
    if (vxpt_get_camera(ctx, 0, camInfo) != VXPT_OK) return fail("reading the camera");
    const float baseYaw = camInfo[30], basePitch = camInfo[31];
    float yaw = baseYaw, pitch = basePitch;

    std::vector<BatchedFrame> batch;
    std::vector<FrameRecord> perf;
    std::string runStamp;
    const size_t frameBytes = (size_t)o.width * o.height * 4 * sizeof(float);
    // a render size that moves: every saved frame is brought to the output size
    const bool resizing = o.dynamicResolution || !o.sizeSchedule.empty();
    const bool upscale = o.renderScale < 1.0f || resizing;
    int curW = o.renderWidth, curH = o.renderHeight, nextW = curW, nextH = curH;
    vxpt_render_params rp{};
    if (vxpt_get_render_params(ctx, &rp) != VXPT_OK) return fail("reading the rendering settings");
    const float targetFps = o.targetFps > 0.0f ? o.targetFps : rp.target_fps;
    if (o.dynamicResolution)
        std::cout << "Dynamic resolution: target " << targetFps << " fps, widths "
                  << std::min(rp.min_render_width, o.renderWidth) << ".." << o.renderWidth << std::endl;

    for (int frame = 0; frame < o.totalFrames; frame++) {  // mainOffline.cpp:273-408
        const int frameNumber = frame + 1;
        const auto t0 = std::chrono::steady_clock::now();
        const float dtMs = std::chrono::duration<float, std::milli>(t0 - last).count();  // Timer::getDeltaTime
        last = t0;
        const bool shouldSave =
            std::find(o.savedFrames.begin(), o.savedFrames.end(), frameNumber) != o.savedFrames.end();
        if (frame == 0) runStamp = timestamp_now();  // PerformanceTracker::beginFrame of the first frame

        // the edit picked last frame reaches the geometry now
        if (editPending) {
            if (vxpt_set_block(ctx, edit[0], edit[1], edit[2], edit[3]) != VXPT_OK) return fail("editing a block");
            editPending = false;
        }
        if (o.removalCircle) {  // mainOffline.cpp:281-305
            if (circleDone < kCircleRemovals) {
                const int dirIndex = circleDone / kPerDirection;
                if (dirIndex != lastDirection) {
                    const float angle = (float)dirIndex * (kTwoPi / (float)kDirections);
                    const float yawOff = (float)(kYawAmp * std::cos(angle)), pitchOff = (float)(kPitchAmp * std::sin(angle));
                    yaw = baseYaw + yawOff;
                    pitch = basePitch + pitchOff;
                    std::cout << "CIRCULAR TEST: Switching to view direction #" << dirIndex + 1 << " (yaw offset "
                              << yawOff << ", pitch offset " << pitchOff << ")" << std::endl;
                    lastDirection = dirIndex;
                }
            } else if (!circleRestored) {
                yaw = baseYaw;
                pitch = basePitch;
                circleRestored = true;
                std::cout << "CIRCULAR TEST: Restored base camera orientation after scripted removals." << std::endl;
            }
            // historyCamera = camera; camera.update() (:278-279, 307)
            if (vxpt_set_camera_angles(ctx, cam.pos, yaw, pitch, cam.fov_deg) != VXPT_OK) return fail("camera");
            std::cout << "CAMERA: frame " << frameNumber << " yaw " << std::hexfloat << yaw << " pitch " << pitch
                      << std::defaultfloat << std::endl;
        }
        if (clickPending) {  // VoxelEngine::update's click, against the world as edited so far
            clickPending = false;
            int blockId;
            if (!clickSequence.empty()) {
                const size_t idx = std::min(clickIndex, clickSequence.size() - 1);
                blockId = clickSequence[idx];
                clickIndex = idx + 1 < clickSequence.size() ? idx + 1 : idx;
            } else {
                static const int defaultSequence[3] = {16, 0, 16};
                blockId = defaultSequence[defaultIndex++ % 3];
            }
            int32_t pk[10];
            if (vxpt_pick_block(ctx, pk) != VXPT_OK) return fail("picking");
            if (blockId == 0 && pk[0]) {
                edit[0] = pk[1]; edit[1] = pk[2]; edit[2] = pk[3]; edit[3] = 0;
                editPending = true;
            } else if (blockId != 0 && pk[5] && pk[0]) {
                edit[0] = pk[6]; edit[1] = pk[7]; edit[2] = pk[8]; edit[3] = blockId;
                editPending = true;
            }
            if (editPending)
                std::cout << "EDIT: frame " << frameNumber << " block " << edit[3] << " at (" << edit[0] << ","
                          << edit[1] << "," << edit[2] << ")" << std::endl;
        }

        if (o.todRange && frame > 0) {  // frame 0's sky is the one set above
            const float tod = o.tod0 + (o.tod1 - o.tod0) * ((float)frame / (float)(o.totalFrames - 1));
            if (set_sky(tod) != VXPT_OK) return fail("building the sky");
        }

        for (const auto &e : o.sizeSchedule)
            if (e.frame == frame) { nextW = e.w; nextH = e.h; }
        if (resizing && (nextW != curW || nextH != curH)) {
            if (vxpt_set_render_size(ctx, nextW, nextH) != VXPT_OK) return fail("setting the render size");
            curW = nextW;
            curH = nextH;
            std::cout << "RENDER SIZE: frame " << frameNumber << " at " << curW << "x" << curH << std::endl;
        }

        const double updateMs = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
        if (vxpt_render_frame(ctx, &dp, frame, o.spp) != VXPT_OK) return fail("rendering");
        const auto tp = std::chrono::steady_clock::now();
        if (vxpt_postprocess(ctx, &pp, dtMs) != VXPT_OK) return fail("post-processing");
        if (shouldSave) {  // storeFrameInBatch (OfflineBackend.cpp:117-131)
            BatchedFrame b;
            b.rgba.resize((size_t)o.width * o.height * 4);
            if (upscale && vxpt_upscale(ctx, o.width, o.height, o.upscaleMode, o.sharpness) != VXPT_OK)
                return fail("upscaling");
            if (vxpt_readback(ctx, upscale ? VXPT_BUF_FRAME_UPSCALED : VXPT_BUF_FRAME, b.rgba.data(), frameBytes) != VXPT_OK)
                return fail("reading the frame");
            b.path = frame_path(o.outputPrefix, frame);
            batch.push_back(std::move(b));
        }
        if (vxpt_sync(ctx) != VXPT_OK) return fail("synchronising");
        const auto t1 = std::chrono::steady_clock::now();
        FrameRecord rec{frameNumber,
                        (shouldSave ? "Saved frame " : "Convergence frame ") + std::to_string(frameNumber) + "/" +
                            std::to_string(o.totalFrames) +
                            (resizing ? " traced at " + std::to_string(curW) + "x" + std::to_string(curH) : std::string()),
                        {}, std::chrono::duration<double, std::milli>(t1 - tp).count(),
                        std::chrono::duration<double, std::milli>(t1 - t0).count(), dtMs, updateMs};
        vxpt_timings(ctx, &rec.t);
        perf.push_back(rec);
        if (o.dynamicResolution) {  // Backend::dynamicResolution on the frame's GPU time; a 16:9 height inside the maximum
            const int minW = std::min(std::max(rp.min_render_width, 16), o.renderWidth);
            if (vxpt_dynres_next_width(curW, rec.t.frame_ms, targetFps, minW, o.renderWidth, &nextW, &nextH) != VXPT_OK)
                return fail("the resolution controller");
            nextH = std::min(std::max(nextH, 1), o.renderHeight);
        }
        // the clicks the reference scripts after a frame (mainOffline.cpp:346-395)
        if (o.removalCircle) {
            if (circleDone < kCircleRemovals) {
                ++circleDone;
                std::cout << "CIRCULAR TEST: Frame " << frameNumber << " deleting block #" << circleDone << std::endl;
                clickPending = true;
            }
        } else if (o.removal20) {
            if (removals < kRemovals20) {
                ++removals;
                std::cout << "REMOVAL TEST: Frame " << frameNumber << " deleting block #" << removals << std::endl;
                clickPending = true;
            }
        } else if (o.testSequence) {
            if (frameNumber == 2 || frameNumber == 5 || frameNumber == 8) clickPending = true;
        }
        if (shouldSave || frameNumber % 16 == 0)
            std::cout << "Frame " << frameNumber << "/" << o.totalFrames << " completed"
                      << (shouldSave ? " (SAVED)" : "") << std::endl;
    }

    // writeAllBatchedFrames (OfflineBackend.cpp:133-184): PNG encoding in parallel on host threads
    std::cout << "\n=== Rendering Complete - Writing all frames to disk ===" << std::endl;
    std::vector<std::future<int>> writers;
    for (const auto &b : batch)
        writers.push_back(std::async(std::launch::async, [&o, &b] {
            return vxpt_write_png_rgba32f(b.path.c_str(), o.width, o.height, b.rgba.data());
        }));
    int writeErrors = 0;
    for (auto &w : writers) writeErrors += w.get() != VXPT_OK;
    if (writeErrors) {
        std::cerr << "Error: " << writeErrors << " frame(s) failed to write" << std::endl;
        vxpt_destroy(ctx);
        return 1;
    }
    std::cout << "Output files saved with prefix: " << o.outputPrefix << std::endl;

    {  // PerformanceTracker::saveReport: the run summary, and the per-frame rows as a CSV
        const std::string csv = o.outputPrefix + "_frames.csv";
        std::ofstream rep(csv);
        rep << "# " << o.runComment << "\n# " << o.width << "x" << o.height << ", " << o.spp << " spp"
            << (resizing ? ", render size per frame in the comment column, starting"
                         : std::string())
            << (upscale ? ", traced at " + std::to_string(o.renderWidth) + "x" + std::to_string(o.renderHeight) : std::string())
            << "\n"
            << "frame,trace_ms,denoise_ms,sky_ms,frame_ms,post_ms,wall_ms,dt_ms,comment\n";
        double sumTrace = 0, sumDen = 0, sumWall = 0;
        for (const auto &r : perf) {
            rep << r.frame << "," << r.t.trace_ms << "," << r.t.denoise_ms << "," << r.t.sky_ms << ","
                << r.t.frame_ms << "," << r.postMs << "," << r.wallMs << "," << std::setprecision(9) << r.dtMs
                << std::setprecision(6) << "," << r.comment << "\n";
            sumTrace += r.t.trace_ms;
            sumDen += r.t.denoise_ms;
            sumWall += r.wallMs;
        }
        const double n = (double)perf.size();
        if (!append_run_summary(o.perfReport, runStamp, o.width, o.height, perf, o.runComment))
            std::cerr << "Warning: cannot write the performance report " << o.perfReport << std::endl;
        std::cout << "\n=== Performance Report ===\n"
                  << "avg path tracing " << sumTrace / n << " ms, denoiser " << sumDen / n << " ms, wall "
                  << sumWall / n << " ms per frame\nPerformance data saved to: " << o.perfReport
                  << " (per frame: " << csv << ")" << std::endl;
    }

    int rc = 0;
    if (o.testCanonical || o.updateCanonical) {  // mainOffline.cpp:423-498
        const std::string testImagePath = frame_path(o.outputPrefix, o.totalFrames - 1);
        if (o.updateCanonical) {
            std::cout << "\n=== Updating Canonical Image ===" << std::endl;
            std::error_code ec;
            if (std::filesystem::copy_file(testImagePath, o.canonicalImagePath,
                                           std::filesystem::copy_options::overwrite_existing, ec))
                std::cout << "Canonical image updated: " << o.canonicalImagePath << std::endl;
            else
                std::cerr << "Failed to update canonical image: " << ec.message() << std::endl;
        }
        if (o.testCanonical) {
            std::cout << "\n=== Canonical Image Testing ===" << std::endl;
            if (!std::filesystem::exists(o.canonicalImagePath)) {
                std::cout << "Warning: Canonical image not found at " << o.canonicalImagePath << "\n"
                          << "Use --update-canonical to create it from current render" << std::endl;
            } else if (!std::filesystem::exists(testImagePath)) {
                std::cerr << "Error: Test image not found at " << testImagePath << std::endl;
            } else {
                std::cout << "Comparing: " << testImagePath << " vs " << o.canonicalImagePath << std::endl;
                vxpt_image_diff_result r{};
                if (vxpt_image_diff(testImagePath.c_str(), o.canonicalImagePath.c_str(), &r) != VXPT_OK) {
                    std::cerr << "Error: image comparison failed" << std::endl;
                    rc = 1;
                } else {
                    print_diff(r);
                    const std::string diffPath = o.outputPrefix + "_diff.png";
                    if (vxpt_image_diff_png(testImagePath.c_str(), o.canonicalImagePath.c_str(),
                                            diffPath.c_str()) == VXPT_OK)
                        std::cout << "Difference visualization saved to: " << diffPath << std::endl;
                    else
                        std::cerr << "Failed to generate difference image" << std::endl;
                    if (!r.is_identical && !r.is_very_close) {
                        std::cout << "\nWarning: Significant differences detected from canonical image!\n"
                                  << "This may indicate a regression or intentional change." << std::endl;
                        if (!r.is_close) std::cout << "Consider investigating the differences." << std::endl;
                    } else {
                        std::cout << "\nImage matches canonical reference within acceptable tolerance." << std::endl;
                    }
                }
            }
        }
    }
    vxpt_destroy(ctx);
    return rc;
}
