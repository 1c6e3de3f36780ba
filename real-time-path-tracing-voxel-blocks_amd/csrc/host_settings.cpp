// vxpt -- host runtime, settings: the YAML reader, the tuning defaults and their ranges, the denoiser's and
// post-process defaults, global_settings.yaml / materials.yaml / blocks.yaml and the scene camera, and the
// parameter and tuning entry points.
#include <algorithm>
#include <cstdlib>
#include <fstream>
#include <map>
#include <sstream>
#include <string>
#include <vector>

#include "host_ctx.hpp"

namespace vx::host {

// minimal YAML reader for the reference's settings / scene / asset files:
// `section:` headers, `key: value` pairs, `- {k: v, ...}` / `properties: {...}` flow maps
std::string trim(const std::string &s) {
    size_t a = s.find_first_not_of(" \t\r\n"), b = s.find_last_not_of(" \t\r\n");
    return a == std::string::npos ? std::string() : s.substr(a, b - a + 1);
}
std::map<std::string, std::string> parse_flow_map(const std::string &s) {
    std::map<std::string, std::string> m;
    size_t a = s.find('{'), b = s.rfind('}');
    if (a == std::string::npos || b == std::string::npos) return m;
    std::string body = s.substr(a + 1, b - a - 1);
    int depth = 0;
    std::string cur;
    std::vector<std::string> items;
    for (char c : body) {
        if (c == '[') depth++;
        if (c == ']') depth--;
        if (c == ',' && depth == 0) { items.push_back(cur); cur.clear(); continue; }
        cur += c;
    }
    if (!trim(cur).empty()) items.push_back(cur);
    for (auto &it : items) {
        size_t c = it.find(':');
        if (c == std::string::npos) continue;
        m[trim(it.substr(0, c))] = trim(it.substr(c + 1));
    }
    return m;
}
std::vector<float> parse_list(const std::string &s) {
    std::vector<float> v;
    std::string t = s;
    for (char &c : t)
        if (c == '[' || c == ']' || c == ',') c = ' ';
    std::istringstream is(t);
    float f;
    while (is >> f) v.push_back(f);
    return v;
}
bool as_bool(const std::string &s) { return s == "true" || s == "1" || s == "True"; }

}  // namespace vx::host

// the measured best schedule; vxpt_set_tuning changes it per context
vxpt_tuning tuning_defaults() {
    vxpt_tuning t{};
    t.dda_boxes = 1;          // empty-box tables: 7.56 -> 7.06 ms of trace per C3 frame (round 3)
    t.box_cap = 32;           // growth limits swept flat (8:8 .. 32:64 within 0.03 ms, round 3); on the round-6 walk
    t.box_cap_up = 32;        // ladder with the direction sort 8:8 -> 32:32 -1.3 % (four runs each)
    t.brick_steps = 3;        // in-brick walks yield after 3 crossings: 6.44 -> 6.26 ms
    t.cam_steps = 10;         // camera rays walk whole bricks
    t.iter_cap = 4;           // caps 4 / 6 / 8 / 12: 7.02 / 6.84 / 7.07 / 7.63 ms (round 2); with the sky exit
                              // (round 6) 5 against 6: 5.439 / 5.438 / 5.440 / 5.463 -> 5.410 / 5.399 / 5.413 / 5.423 ms
    t.iter_cap2 = 6;          // a second level after 6 more iterations (round 2-6: 16, its walks in resume_split
                              // pieces: 5.74 -> 5.66-5.68 ms; one lane per walk at that level: 7.59 ms, round 2)
    t.iter_cap3 = 12;         // round 6: a third level, 12 more iterations, before the pieces: the ladder 4 / 6 / 12
                              // against 5 / 16: 5.46 -> 5.20 ms per C3 frame (four runs each)
    t.resume_wg_per_cu = 24;  // 4 / 8 / 16 / 32: 6.96 / 6.85 / 6.84 / 6.87 ms (round 2); on the round-6 walk ladder
                              // 16 -> 24: 5.195 -> 5.168 ms (four runs each, every run faster)
    t.sort_mode = 2;          // direction-class sort (octant x dominant axis): until round 6 1.5 % faster traversal,
                              // paid back by the producers; on the walk ladder 5.188 -> 5.156 ms (sort 1), with 32-brick
                              // boxes 5.150 -> 5.067 ms (four runs each)
    t.overlap = 1;            // pass halves on two streams: 6.84 -> 6.06 ms
    t.state_sets = 3;         // 3 sets: 5.409 -> 5.394 ms (four interleaved runs each, every run faster; round 5)
    t.firefly_fused = 1;      // -4 us per chain
    t.ta_supertiles = 1;      // temporal pass traffic 351 -> 266 MB per frame
    t.hf_split = 4;           // 16.3 -> 11.8 us history fix (with readlane sums)
    t.stencil_tile = 16;      // 32x32 tiles: 50.0 -> 55.8 / 48.5 -> 52.4 us
    t.lds_bricks = 0;
    t.resume_split = 16;      // (with iter_cap2 0: every straggler in pieces, 5.73 -> 6.7-9.2 ms)
    t.later_split = 16;       // 4/4 bounces: 16.39 -> 15.67 ms per frame (3/1 has no later segments)
    t.restir_waves = 0;       // 4 waves: whole frames slower (Appendix A); see bench.band_tuning for bands
    t.ghost_rows = 1;         // bands: the chain's ordered exchange groups 7 -> 3 per frame
    t.chain_gate = 1;         // the chain alone on the GPU (its roofline); bench.band_tuning: 0 for bands
    t.sky_exit = 1;           // C3 frame 5.443 -> 5.419 ms (two runs each, both faster); one band 1-2 %
    t.xcd_order = 0;
    t.iter_cap4 = 0;          // a fourth level: 4 / 8 / 16 / 6-8-12 ladders 5.26-5.27 ms, no gain
    t.brick_pass = 1;         // visibility walks cross occupied bricks with no cube ahead as empty boxes:
                              // C3 frame 5.09-5.10 -> 4.85-4.87 ms, interleaved with the parent
    t.front_streams = 2;      // first halves of consecutive passes side by side: 5.89 -> 5.76 ms per C3
                              // frame; one 136-row band 1.95 -> 1.63 ms (1.56 with 3 state sets)
    return t;
}
bool tuning_valid(const vxpt_tuning &t) {
    auto in = [](int v, int lo, int hi) { return v >= lo && v <= hi; };
    return in(t.dda_boxes, 0, 1) && in(t.box_cap, 1, 255) && in(t.box_cap_up, 1, 255) && in(t.brick_steps, 1, 64) &&
           in(t.cam_steps, 1, 64) && in(t.iter_cap, 1, 1024) && in(t.iter_cap2, 0, 1024) &&
           in(t.resume_wg_per_cu, 1, 64) && in(t.sort_mode, 0, 2) && in(t.overlap, 0, 1) &&
           in(t.state_sets, 2, kMaxSets) && in(t.firefly_fused, 0, 1) && in(t.ta_supertiles, 0, 1) &&
           in(t.hf_split, 1, 16) && (t.stencil_tile == 16 || t.stencil_tile == 32) && in(t.front_streams, 1, kMaxSets) &&
           in(t.lds_bricks, 0, 1) && (t.resume_split == 1 || t.resume_split == 2 || t.resume_split == 4 ||
                                       t.resume_split == 8 || t.resume_split == 16) &&
           (t.later_split == 1 || t.later_split == 2 || t.later_split == 4 || t.later_split == 8 || t.later_split == 16) &&
           (t.restir_waves == 0 || t.restir_waves == 4) && in(t.ghost_rows, 0, 1) &&
           in(t.chain_gate, 0, 1) && in(t.sky_exit, 0, 1) && in(t.xcd_order, 0, 7) && in(t.iter_cap3, 0, 1024) && in(t.iter_cap4, 0, 1024) &&
           in(t.brick_pass, 0, 1);
}

namespace vx::host {

// GlobalSettings.h:10-186 defaults (the reference yaml overrides most of them: vxpt_load_settings)
vxpt_post_params default_post() {
    vxpt_post_params p{};
    p.manual_exposure = 10.0f; p.tone_mapping_curve = 0; p.white_point = 10.0f;
    p.contrast = 1.0f; p.saturation = 1.0f; p.lift = 0.0f; p.gain = 1.0f;
    p.enable_bloom = 1; p.bloom_threshold = 1.0f; p.bloom_intensity = 0.15f; p.bloom_radius = 2.0f;
    p.enable_auto_exposure = 1; p.exposure_speed = 1.0f; p.exposure_min = -8.0f; p.exposure_max = 8.0f;
    p.exposure_compensation = 0.0f; p.histogram_min_percent = 40.0f; p.histogram_max_percent = 80.0f;
    p.target_luminance = 0.18f;
    p.enable_vignette = 0; p.vignette_strength = 0.5f; p.vignette_radius = 0.8f; p.vignette_smoothness = 0.5f;
    p.enable_lens_flare = 0; p.lens_flare_intensity = 0.00001f; p.lens_flare_ghost_spacing = 0.15f;
    p.lens_flare_ghost_count = 4; p.lens_flare_halo_radius = 0.1f; p.lens_flare_sun_size = 0.006f;
    p.lens_flare_distortion = 0.015f;
    p.draw_crosshair = 1;
    return p;
}

const vxpt_denoise_params &default_denoise() {
    static vxpt_denoise_params d{30.f, 6.f, 2.f, 0.5f, 0.15f, 0.003f, 0.01f, 0.05f, 500000.f, 1, 1, 1, 1, 1, 1, 0, 0};
    return d;
}

}  // namespace vx::host

extern "C" {

int vxpt_load_settings(vxpt_ctx *c) {
    if (!c) return VXPT_ERR_ARG;
    // global_settings.yaml: denoising + sky sections (GlobalSettings.cpp:69-492)
    std::ifstream f(c->dataDir + "/settings/global_settings.yaml");
    if (!f) return fail(c, VXPT_ERR_IO, "missing settings/global_settings.yaml");
    vxpt_denoise_params d = default_denoise();
    vxpt_post_params pp = default_post();
    std::string line, section;
    while (std::getline(f, line)) {
        const size_t hash = line.find('#');
        if (hash != std::string::npos) line = line.substr(0, hash);
        if (trim(line).empty()) continue;
        const bool indented = line[0] == ' ' || line[0] == '\t';
        const size_t col = line.find(':');
        if (col == std::string::npos) continue;
        const std::string key = trim(line.substr(0, col)), val = trim(line.substr(col + 1));
        if (!indented) { section = key; continue; }
        if (section == "denoising") {
            const float v = (float)std::atof(val.c_str());
            if (key == "enableTemporalAccumulation") d.enable_temporal_accumulation = as_bool(val);
            else if (key == "enableHistoryFix") d.enable_history_fix = as_bool(val);
            else if (key == "enableHistoryClamping") d.enable_history_clamping = as_bool(val);
            else if (key == "enableSpatialFiltering") d.enable_spatial_filtering = as_bool(val);
            else if (key == "enableFireflyFilter") d.enable_firefly_filter = as_bool(val);
            else if (key == "enableHitDistanceReconstruction") d.enable_hit_distance_reconstruction = as_bool(val);
            else if (key == "enablePrePass") d.enable_pre_pass = as_bool(val);
            else if (key == "maxAccumulatedFrameNum") d.max_accumulated_frame_num = v;
            else if (key == "maxFastAccumulatedFrameNum") d.max_fast_accumulated_frame_num = v;
            else if (key == "phiLuminance") d.phi_luminance = v;
            else if (key == "lobeAngleFraction") d.lobe_angle_fraction = v;
            else if (key == "roughnessFraction") d.roughness_fraction = v;
            else if (key == "depthThreshold") d.depth_threshold = v;
            else if (key == "atrousIterationNum") d.atrous_iteration_num = (int)v;
            else if (key == "disocclusionThreshold") d.disocclusion_threshold = v;
            else if (key == "disocclusionThresholdAlternate") d.disocclusion_threshold_alternate = v;
            else if (key == "denoisingRange") d.denoising_range = v;
        } else if (section == "postprocess") {  // GlobalSettings.cpp:277-355
            const float v = (float)std::atof(val.c_str());
            const int b = as_bool(val) ? 1 : 0;
            if (key == "manualExposure") pp.manual_exposure = v;
            else if (key == "toneMappingCurve") pp.tone_mapping_curve = (int)v;
            else if (key == "whitePoint") pp.white_point = v;
            else if (key == "contrast") pp.contrast = v;
            else if (key == "saturation") pp.saturation = v;
            else if (key == "gain") pp.gain = v;
            else if (key == "lift") pp.lift = v;
            else if (key == "enableBloom") pp.enable_bloom = b;
            else if (key == "bloomThreshold") pp.bloom_threshold = v;
            else if (key == "bloomIntensity") pp.bloom_intensity = v;
            else if (key == "bloomRadius") pp.bloom_radius = v;
            else if (key == "enableAutoExposure") pp.enable_auto_exposure = b;
            else if (key == "exposureSpeed") pp.exposure_speed = v;
            else if (key == "exposureMin") pp.exposure_min = v;
            else if (key == "exposureMax") pp.exposure_max = v;
            else if (key == "exposureCompensation") pp.exposure_compensation = v;
            else if (key == "histogramMinPercent") pp.histogram_min_percent = v;
            else if (key == "histogramMaxPercent") pp.histogram_max_percent = v;
            else if (key == "targetLuminance") pp.target_luminance = v;
            else if (key == "enableVignette") pp.enable_vignette = b;
            else if (key == "vignetteStrength") pp.vignette_strength = v;
            else if (key == "vignetteRadius") pp.vignette_radius = v;
            else if (key == "vignetteSmoothness") pp.vignette_smoothness = v;
            else if (key == "enableLensFlare") pp.enable_lens_flare = b;
            else if (key == "lensFlareIntensity") pp.lens_flare_intensity = v;
            else if (key == "lensFlareGhostSpacing") pp.lens_flare_ghost_spacing = v;
            else if (key == "lensFlareGhostCount") pp.lens_flare_ghost_count = (int)v;
            else if (key == "lensFlareHaloRadius") pp.lens_flare_halo_radius = v;
            else if (key == "lensFlareSunSize") pp.lens_flare_sun_size = v;
            else if (key == "lensFlareDistortion") pp.lens_flare_distortion = v;
        } else if (section == "sky") {
            const float v = (float)std::atof(val.c_str());
            if (key == "timeOfDay") c->skyParams[0] = v;
            else if (key == "sunAxisAngle") c->skyParams[1] = v;
            else if (key == "sunAxisRotate") c->skyParams[2] = v;
            else if (key == "skyBrightness") c->skyParams[3] = v;
        }
    }
    c->yamlDenoise = d;
    c->yamlPost = pp;
    if (int r = vxpt_read_render_params((c->dataDir + "/settings/global_settings.yaml").c_str(), &c->renderParams))
        return fail(c, r, "cannot read the rendering settings");
    // materials.yaml (order == material index, MaterialManager.cpp:84-97) + blocks.yaml
    std::ifstream fm(c->dataDir + "/assets/materials.yaml");
    if (!fm) return fail(c, VXPT_ERR_IO, "missing assets/materials.yaml");
    std::vector<std::string> ids;
    std::vector<std::map<std::string, std::string>> props, texs;
    while (std::getline(fm, line)) {
        const std::string tl = trim(line);
        if (tl.rfind("- id:", 0) == 0) {
            ids.push_back(trim(tl.substr(5)));
            props.emplace_back();
            texs.emplace_back();
        } else if (tl.rfind("properties:", 0) == 0 && !props.empty()) {
            props.back() = parse_flow_map(tl);
        } else if (tl.rfind("textures:", 0) == 0 && !texs.empty()) {
            texs.back() = parse_flow_map(tl);
        }
    }
    std::ifstream fb(c->dataDir + "/assets/blocks.yaml");
    if (!fb) return fail(c, VXPT_ERR_IO, "missing assets/blocks.yaml");
    while (std::getline(fb, line)) {
        const std::string tl = trim(line);
        if (tl.rfind("- {", 0) != 0) continue;
        auto m = parse_flow_map(tl);
        const int bid = std::atoi(m["id"].c_str());
        if (bid < 1 || bid > 12) continue;
        const auto it = std::find(ids.begin(), ids.end(), m["material"]);
        if (it == ids.end()) continue;
        const int mi = (int)(it - ids.begin());
        auto &p = props[mi];
        MatDev md{{1.f, 1.f, 1.f}, 0.5f, 0.0f, 0, mi, 0};  // MaterialProperties defaults (MaterialDefinition.h:18-28)
        if (p.count("roughness")) md.roughness = (float)std::atof(p["roughness"].c_str());
        if (p.count("metallic")) md.metallic = std::atof(p["metallic"].c_str()) != 0.0;
        if (p.count("translucency")) md.translucency = (float)std::atof(p["translucency"].c_str());
        if (p.count("is_thinfilm")) md.thin = as_bool(p["is_thinfilm"]);
        if (p.count("albedo")) {
            auto v = parse_list(p["albedo"]);
            if (v.size() == 3) { md.albedo[0] = v[0]; md.albedo[1] = v[1]; md.albedo[2] = v[2]; }
        }
        if (p.count("uv_scale")) md.uvScale = (float)std::atof(p["uv_scale"].c_str());
        if (p.count("use_world_grid_uv")) md.worldGridUV = as_bool(p["use_world_grid_uv"]) ? 1 : 0;
        static const char *kTexKeys[4] = {"albedo", "normal", "roughness", "metallic"};
        for (int k = 0; k < 4; ++k) c->texPath[bid][k] = texs[mi].count(kTexKeys[k]) ? texs[mi][kTexKeys[k]] : "";
        c->mats[bid] = md;
    }
    return VXPT_OK;
}

int vxpt_load_scene_camera(vxpt_ctx *c, const char *path, vxpt_camera *out) {
    if (!c || !out) return VXPT_ERR_ARG;
    std::string p = path ? path : (c->dataDir + "/scene/scene_export.yaml");
    std::ifstream f(p);
    if (!f) return fail(c, VXPT_ERR_IO, "cannot open " + p);
    std::string line, section;
    vxpt_camera cam{{35.6184f, 11.8733f, 42.0387f}, {-0.321564f, -0.0129988f, -0.946799f}, 90.0f};
    while (std::getline(f, line)) {
        const size_t hash = line.find('#');
        if (hash != std::string::npos) line = line.substr(0, hash);
        if (trim(line).empty()) continue;
        const size_t col = line.find(':');
        if (col == std::string::npos) continue;
        const std::string key = trim(line.substr(0, col)), val = trim(line.substr(col + 1));
        if (line[0] != ' ') { section = key; continue; }
        if (section != "camera") continue;
        auto v = parse_list(val);
        if (key == "position" && v.size() == 3) std::copy(v.begin(), v.end(), cam.pos);
        else if (key == "direction" && v.size() == 3) std::copy(v.begin(), v.end(), cam.dir);
        else if (key == "fov" && v.size() == 1) cam.fov_deg = v[0];
    }
    *out = cam;
    return VXPT_OK;
}

int vxpt_get_denoise_params(vxpt_ctx *c, vxpt_denoise_params *out) {
    if (!c || !out) return VXPT_ERR_ARG;
    *out = c->yamlDenoise;
    return VXPT_OK;
}

int vxpt_get_post_params(vxpt_ctx *c, vxpt_post_params *out) {
    if (!c || !out) return VXPT_ERR_ARG;
    *out = c->yamlPost;
    return VXPT_OK;
}

int vxpt_read_render_params(const char *path, vxpt_render_params *out) {
    if (!path || !out) return VXPT_ERR_ARG;
    std::ifstream f(path);
    if (!f) return VXPT_ERR_IO;
    vxpt_render_params rp{60.0f, 0, 480, 270, 2560, 1440};  // GlobalSettings.h:316-325
    std::string line, section;
    while (std::getline(f, line)) {
        const size_t hash = line.find('#');
        if (hash != std::string::npos) line = line.substr(0, hash);
        if (trim(line).empty()) continue;
        const size_t col = line.find(':');
        if (col == std::string::npos) continue;
        const std::string key = trim(line.substr(0, col)), val = trim(line.substr(col + 1));
        if (line[0] != ' ' && line[0] != '\t') { section = key; continue; }
        if (section != "rendering") continue;  // GlobalSettings.cpp:433-451: the controller's keys
        if (key == "targetFPS") rp.target_fps = (float)std::atof(val.c_str());
        else if (key == "dynamicResolution") rp.dynamic_resolution = as_bool(val) ? 1 : 0;
        else if (key == "minRenderWidth") rp.min_render_width = std::atoi(val.c_str());
        else if (key == "minRenderHeight") rp.min_render_height = std::atoi(val.c_str());
        else if (key == "maxRenderWidth") rp.max_render_width = std::atoi(val.c_str());
        else if (key == "maxRenderHeight") rp.max_render_height = std::atoi(val.c_str());
    }
    *out = rp;
    return VXPT_OK;
}

int vxpt_get_render_params(vxpt_ctx *c, vxpt_render_params *out) {
    if (!c || !out) return VXPT_ERR_ARG;
    *out = c->renderParams;
    return VXPT_OK;
}

int vxpt_tuning_defaults(vxpt_tuning *out) {
    if (!out) return VXPT_ERR_ARG;
    *out = tuning_defaults();
    return VXPT_OK;
}

int vxpt_get_tuning(vxpt_ctx *c, vxpt_tuning *out) {
    if (!c || !out) return VXPT_ERR_ARG;
    *out = c->tune;
    return VXPT_OK;
}

int vxpt_set_tuning(vxpt_ctx *c, const vxpt_tuning *t) {
    if (!c || !t) return VXPT_ERR_ARG;
    if (!tuning_valid(*t)) return fail(c, VXPT_ERR_ARG, "tuning field out of range");
    HIPCHK(c, hipSetDevice(c->dev));
    // whatever is in flight used the old schedule's buffers
    for (hipStream_t fs : c->frontStreams) HIPCHK(c, hipStreamSynchronize(fs));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    const bool tables = t->dda_boxes != c->tune.dda_boxes || t->box_cap != c->tune.box_cap ||
                        t->box_cap_up != c->tune.box_cap_up;
    c->tune = *t;
    c->nSets = t->state_sets;
    c->useBoxes = t->dda_boxes != 0;
    c->boxCap = t->box_cap;
    c->boxCapUp = t->box_cap_up;
    if (tables && c->useBoxes && c->nBricks > 0 && c->worldBuild == VXPT_WORLD_BUILD_DEVICE) {
        if (int r = device_tables(c)) return r;
    } else if (tables && c->useBoxes && c->nBricks > 0) {  // the current world's box tables, rebuilt whole
        const int BX = c->cx * 8, BY = c->cy * 8, BZ = c->cz * 8;
        brick_prefix(c);
        c->hBox.assign((size_t)8 * c->nBricks, 0u);
        for (int oct = 0; oct < 8; ++oct) box_fill(c, oct, 0, BX - 1, 0, BY - 1, 0, BZ - 1);
        if (int r = upload_vec(c, c->bbox, c->hBox.data(), c->hBox.size())) return r;
        HIPCHK(c, hipStreamSynchronize(c->stream));
    }
    return VXPT_OK;
}

}  // extern "C"
