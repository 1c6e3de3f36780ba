// vxpt -- the one internal header of the host runtime (vxpt_host.cpp, host_settings.cpp, host_world.cpp, host_sky.cpp,
// host_textures.cpp, host_instances.cpp, host_frame.cpp, host_bands.cpp, host_terrain.cpp, host_resize.cpp) behind the C ABI (include/vxpt.h):
// the context, its allocation helpers, and the host functions that are called across files.
//
// The library is built with default visibility: everything in vx::host is declared hidden here, so
// that none of it becomes a dynamic symbol of libvxpt.so.  A function used by one file only stays in
// an anonymous namespace in that file.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <array>
#include <cstdint>
#include <map>
#include <string>
#include <vector>

#include "../../include/vxpt.h"
#include "box_tables.hpp"
#include "light_map.hpp"
#include "vx_internal.hpp"

typedef struct ncclComm *ncclComm_t;  // <rccl/rccl.h>'s opaque handle (host_bands.cpp, vxpt_destroy)

using namespace vx;

#pragma GCC visibility push(hidden)
namespace vx::host {

// ---------------------------------------------------------------- helpers
template <class T>
struct DBuf {
    T *p = nullptr;
    size_t n = 0;
};

struct GSlot {
    float4 *normalRough = nullptr, *geoNormalThin = nullptr, *albedo = nullptr, *matParam = nullptr;
    float *depth = nullptr, *material = nullptr;
    float4 *rec = nullptr;  // ReSTIR tap records (GBuf::rec), 2 float4 per pixel
    bool recStale = false;  // the planes were written from the host since the records were
};

constexpr int kBlockTypes = 30;  // BlockTypeNum (generated/voxelengine/BlockType.h:39)
constexpr int kPostHist = 257;   // 256 luminance bins + the lens flare's sun flag
constexpr int kMaxSets = 3;      // wavefront state sets (vxpt_ctx::nSets; 4 measured slower on bands)

}  // namespace vx::host
#pragma GCC visibility pop


using namespace vx::host;

vxpt_tuning tuning_defaults();  // host_settings.cpp; exported by name like the functions at the end

struct vxpt_ctx {
    int W = 0, H = 0, dev = 0, rowBegin = 0, rowEnd = 0;
    // dynamic resolution (vxpt_set_render_size; host_resize.cpp): W x H is the render size, maxW x maxH the
    // created one, which every per-pixel allocation is sized for
    int maxW = 0, maxH = 0;
    int totalBounce = 3, diffuseBounce = 1;
    std::string dataDir;
    std::string err;
    hipStream_t stream = nullptr;
    hipEvent_t ev[8] = {};
    hipEvent_t runEv[2] = {};  // around a banded vxpt_render_frames run
    vxpt_timing timing{};
    vxpt_tuning tune = tuning_defaults();

    // scene
    int cx = 0, cy = 0, cz = 0;
    DBuf<uint8_t> voxels;
    DBuf<uint8_t> bricks;
    DBuf<uint64_t> macro, cellMask;
    DBuf<uint8_t> bdist;
    // optional empty-box skip tables (vxpt_tuning.dda_boxes; box_tables.hpp)
    bool useBoxes = tune.dda_boxes != 0;
    BrickPrefix brickPrefix;
    int boxCap = tune.box_cap, boxCapUp = tune.box_cap_up;  // box growth limits (box_tables.hpp)
    std::vector<uint32_t> hBox;
    DBuf<uint32_t> bbox;
    int nBricks = 0;
    uint64_t top = 0;
    int topValid = 0;
    // sky exit (WorldDev::skyTop): per brick column 1 + its highest cube cell row (edits raise it, never
    // lower it: a bound), and its suffix maxima per x / z direction quadrant (the device table)
    std::vector<uint16_t> colTop, hSkyTop;
    DBuf<uint16_t> skyTop;
    // host mirrors of the world: picking, incremental edits, chunk files (the device copies are
    // updated from them in place)
    std::vector<uint8_t> hIds, hBricks, hOd;
    std::vector<uint64_t> hMacro, hCell;
    std::vector<int> topCount;  // cube cells per 64^3 block
    std::vector<uint8_t> hNonAir;  // non-air cells (any id, instanced ones too) per 4^3 brick (brick_lin order)
    // how far an instanced block's mesh reaches outside its cell (the largest vertex overhang of the
    // loaded meshes, at least 1): nearest_surface grows every non-air cell by it
    float meshGrow = 1.0f;
    // world edits / uploads so far, and the last nearest-surface search (band halos of a moving
    // camera): a later position p reuses it as nearDist - |p - nearPos| (1-Lipschitz) while the
    // world is unchanged and that keeps >= 3/4 of the searched distance
    unsigned worldVersion = 0, nearVersion = ~0u;
    V3 nearPos{0.0f, 0.0f, 0.0f};
    float nearDist = 0.0f;
    int prevSceneEmpty = 0;     // the next trace pass's temporal visibility sees no previous scene
    // tables built and edited on the device (vxpt_set_world_build; world.hip): the build's own device state
    // (column tops as a 32-bit plane, prefix counts of occupied bricks); two pinned staging buffers for
    // the edit batches' records, each reused only after the event behind the kernel that read it; the
    // event recorded behind every build / edit (the front streams wait for it); and the events around
    // the last build's / edit's kernels (vxpt_world_build_ms).  hOd, hBox and brickPrefix stay empty
    int worldBuild = VXPT_WORLD_BUILD_HOST;
    DBuf<uint32_t> dColTop;
    DBuf<int> dPrefix;
    WbRec *editStage[2] = {};
    size_t editCap[2] = {};
    hipEvent_t editDone[2] = {};
    bool editUsed[2] = {};
    int editNext = 0;
    hipEvent_t worldWritten = nullptr, wbEv[2] = {};
    bool wbTimed = false;
    // terrain generated on the device (vxpt_generate_terrain_ex; terrain.hip): the permutation table, the
    // window's height plane, the two counts k_terrain_mirrors adds for the host mirrors, and the events
    // around the last call's height, fill and table kernels and its readback (vxpt_terrain_ms)
    DBuf<uint8_t> terPerm, dNonAir;
    DBuf<float> terHeight;
    DBuf<int> dTopCount;
    hipEvent_t terEv[5] = {};
    bool terTimed = false;
    MatDev mats[32] = {};  // by block id: 1..12 cubes (kernel arguments), 13..29 instanced meshes (meshMats)
    CamDev cam{}, prevCam{};
    float camYaw = 0, camPitch = 0;
    // what the two cameras were made from (make_camera_angles' arguments): a resize makes them again at the
    // new size.  heldW x heldH (0: none): the size the history was rendered at, set by a resize that changed
    // the aspect ratio -- until the next frame's denoiser is enqueued the previous camera is a view of that
    // aspect at the new resolution (the view the resampled history holds); do_denoise then makes it again
    // at the render size (release_held_camera)
    struct CamSrc { float pos[3] = {0.f, 0.f, 0.f}, yaw = 0.f, pitch = 0.f, fov = 90.f; bool set = false; };
    CamSrc camSrc, prevCamSrc;
    int heldW = 0, heldH = 0;

    // sky
    DBuf<float4> sky, sun;
    DBuf<float> skyPdf, sunPdf;
    DBuf<AliasBin> skyAlias, sunAlias;
    std::vector<AliasBin> hSkyAlias;
    V3 sunDir;
    float tabSky[540], tabSkyRad[60];
    DBuf<float> solar, limb;
    bool skyReady = false;
    // device sky build (vxpt_set_sky_device) and the alias probe: the alias kernels' scratch, the
    // builds' heads (0 upper-hemisphere sum, 1 sky table, 2 sun table, 3 probe) in device memory and
    // the pinned host copy of the first three, and the event recorded behind a build (the front
    // streams wait for it; the host waits for it before it reads the heads or the build's time)
    AliasScratch aliasScratch;
    AliasHead *skyHeads = nullptr, *hSkyHeads = nullptr;
    hipEvent_t skyWritten = nullptr;
    bool skyDevice = false;   // the tables are the device build's (hSkyAlias is filled on demand)
    bool skyPending = false;  // heads and build time of the last device build not read yet

    // textures (materials.yaml `textures`, TextureManager): per block the albedo / normal /
    // roughness / metallic paths, the loaded RGBA8 mip chains and their table
    std::string texPath[13][4];
    DBuf<uchar4> texels;
    DBuf<TexInfo> texTable;
    std::vector<TexInfo> hTex;
    size_t nTexels = 0;
    int texEnabled = 0;
    // block-compressed texture set (vxpt_load_textures_bc): hTexBc is filled for every such load, the
    // device buffers only when the sampler decodes blocks (texBcOn; not with VXPT_TEX_EXPAND)
    DBuf<uint8_t> texBlocks;
    DBuf<TexBcInfo> texBcTable;
    std::vector<TexBcInfo> hTexBc;
    size_t nTexBlockBytes = 0;
    bool texBcOn = false;
    // the events around the last device encode's kernels (vxpt_bc_encode_ms), created on first use
    hipEvent_t bcEv[2] = {};
    bool bcTimed = false;

    // instanced block meshes and their emissive-triangle lights
    struct BlockDef {
        std::string model;
        bool instanced = false, baseLight = false, emissive = false;
        int lightBase = 0;
        float emission[3] = {0.f, 0.f, 0.f};
        int triangles = 0;             // of the loaded mesh (0: missing file)
        std::vector<float> pos, uv;    // 9 / 6 floats per triangle, object space
    };
    bool modelsLoaded = false;
    BlockDef blocks[kBlockTypes];
    std::vector<int32_t> instances;    // (objectId, instanceId, x, y, z) by object, then instance id
    std::vector<uint32_t> lightMap;    // (instanceId, first light, triangles) per emissive instance
    DBuf<LightInfo> lights;
    DBuf<AliasBin> lightAlias;
    DBuf<float> lightTri, lightWeight;
    DBuf<int> lightInst;
    unsigned nLights = 0;
    float localLightLum = 0.0f;
    // light-update state (Scene.h:91-115): the update type, the edits' instance sets, the instance ->
    // (first light, count) table of the last incremental update, and the remap the next pass applies
    LightUpdateState lightState;
    unsigned prevNumLights = 0;
    int lightsDirty = 0;
    DBuf<int> lightRemap;
    // two-level BVH of the instanced meshes (meshes.hip): BLAS per block type, TLAS per world
    std::vector<BvhNode> hBlas;
    std::vector<float> hBlasTri;
    std::vector<int> hBlasTriId;
    std::vector<int2> hRoot;  // per block type: (first node, first triangle), -1 = no mesh
    DBuf<BvhNode> blas, tlas;
    DBuf<float> blasTri;
    DBuf<int> blasTriId;
    DBuf<int2> blasRoot;
    DBuf<MeshInst> meshInst;
    int nMeshInst = 0;
    // the path kernels' view of the meshes: texcoords in BLAS leaf order, per instance row its cell +
    // block and first light, materials by block id
    std::vector<float> hBlasUV;
    DBuf<float> blasUV;
    DBuf<int4> meshRow;
    DBuf<int> meshRowLight;
    DBuf<MatDev> meshMats;
    MatDev meshMatsUp[32] = {};  // what meshMats holds (uploaded when the materials change)
    // instance refresh on the device (vxpt_set_instance_build; instances.hip): the instance set kept
    // under edits (collect_instances' per-object map; valid while instSetValid), what an edit batch
    // left to enqueue (instDirty: tables, instLightsDirty: light tables too, hRemap: the last light
    // update's remap), the pinned staging pool (two buffers, more only while both are still being read;
    // each reused only after the event behind its copies), the LBVH scratch, the light table's head
    // (its fsum is the luminance sum, fetched on demand), the event behind a refresh (the front streams
    // wait for it) and the events around its kernels.  ibStats: vxpt_instance_build_stats
    int instBuild = VXPT_INSTANCE_BUILD_HOST;
    std::map<int, std::map<unsigned, std::array<unsigned, 3>>> instSet;
    bool instSetValid = false;
    bool instDirty = false, instLightsDirty = false, instBatch = false;
    std::vector<int> hRemap;
    struct InstStage { char *p = nullptr; size_t cap = 0; hipEvent_t done = nullptr; bool used = false; };
    std::vector<InstStage> instStage;
    DBuf<int> lbMiRow, lbSlotInner, lbSlotLeaf, lbVisits;
    DBuf<uint64_t> lbPacked;
    DBuf<float> lbPrimBox, lbExact;
    int nTlasNodes = 0;
    AliasHead *lightHead = nullptr;
    bool lightLumOnDevice = false;
    hipEvent_t instWritten = nullptr, ibEv[2] = {};
    bool ibTimed = false;
    uint32_t ibStats[4] = {};
    // vxpt_mesh_probe / vxpt_mesh_occluded scratch (grown to the largest call)
    DBuf<float> probeRays, probeOut;
    DBuf<int> probeIds;
    DBuf<unsigned char> probeOcc;

    // blue noise
    DBuf<uint8_t> bnSobol, bnScramble, bnRank;

    // frame buffers
    // G-buffer ring of 3 slots: every trace pass writes a slot that is neither
    // the previous pass's (its ReSTIR history) nor the denoiser's history slot
    // (the previous frame's final G-buffer, Denoiser.cu:394-407), so the frame
    // end hands the last slot to the denoiser by index instead of copying planes.
    // Two more slots let first halves (camera rays .. NEE visibility, which read no previous pass)
    // run ahead while up to two second halves still read their previous passes' slots, and one more
    // keeps the denoiser's previous history slot (histOld) out of the pipelined next frame's reach.
    GSlot gb[6];
    int last = 0;              // slot of the most recent trace output
    int tracePrev = 0;         // slot the most recent trace read as its previous pass
    int tracePrev2 = 0;        // the one before (read by the second half before that)
    int hist = 2;              // denoiser history slot (zero at frame 0)
    int histOld = 2;           // the one before (the history of the most recently enqueued denoiser run)
    float4 *illum = nullptr;   // the most recent pass's radiance (one of illumSet)
    float4 *illumSet[kMaxSets] = {};  // per wavefront state set
    float4 *accum = nullptr, *motion = nullptr;
    float4 *accumBuf[2] = {};  // accum alternates between these per accumulation (first pass picks the other)
    // the motion plane holds only zeros (allocated zeroed; the trace stores zeros, the world is static)
    // until a host write: the trace then skips its zero stores
    bool motionZero = true;
    Reservoir *res = nullptr;  // 2*W*H
    float4 *ping = nullptr, *pong = nullptr, *prevIllum = nullptr, *prevFast = nullptr, *output = nullptr;
    float *clampDbg = nullptr;  // vxpt_debug_clamp_decisions (written while clampDbgOn)
    bool clampDbgOn = false;
    float *histLen = nullptr, *prevHistLen = nullptr;
    float4 *wpos = nullptr;
    uint32_t *ffCount = nullptr, *ffIndex = nullptr, *hfList = nullptr, *hfCount = nullptr, *ffCandCount = nullptr;
    uint4 *ffCand = nullptr;
    float4 *ffColor = nullptr;
    Reservoir *ffRes = nullptr;
    bool denoiseInputIsAccum = false;
    // dynamic resolution: the planes outside the G-buffer ring that outlive a frame are resampled into these
    // shadows (allocated at the first size change) and exchange pointers with them; hostWrote: a per-pixel
    // buffer was uploaded (with no pass and no upload yet, a resize only sets the size); rzEv: around the
    // last resample's kernels
    float4 *shPrevIllum = nullptr, *shPrevFast = nullptr, *shMotion = nullptr;
    float *shHistLen = nullptr, *shPrevHistLen = nullptr;
    Reservoir *shRes = nullptr;
    bool hostWrote = false;
    hipEvent_t rzEv[2] = {};
    bool rzTimed = false;
    vxpt_render_params renderParams{60.0f, 0, 480, 270, 2560, 1440};  // GlobalSettings.h:316-325
    // Wavefront state sets, used round-robin by pass: first halves (k_closest .. the RIS
    // visibility rays) run in order on frontStream, each after the pass that last used its set;
    // second halves (temporal reuse, its rays, k_finish, later segments, the spp accumulation) run
    // in order on the context stream, each after its first half.  With 3 sets a first half may
    // start while the two previous second halves are still running.
    int nSets = 2;
    WaveBufs wb[kMaxSets]{};
    size_t wbSlots[kMaxSets] = {};
    int passCount = 0;         // trace passes so far (set = passCount % nSets)
    int lastSet = 0;           // the set of the most recent pass
    // first halves: on front_streams streams by state set (set % front_streams), so a first half may run
    // beside the previous passes' first halves (it reads nothing a first half writes: the waits on
    // backDone order it behind its set's last user only)
    hipStream_t frontStreams[kMaxSets] = {};
    hipEvent_t frontDone[kMaxSets] = {}, backDone[kMaxSets] = {}, frontGate = nullptr;
    std::vector<hipEvent_t> chainEv;  // vxpt_render_frames: around each frame's denoiser chain
    int numCU = 256;
    std::vector<void *> allocs;

    // post-processing (PostProcessor / PostProcessingPipeline): working, bloom and frame
    // planes, luminance histogram, device exposure state
    vxpt_post_params yamlPost{};
    float4 *bloomA = nullptr, *bloomB = nullptr, *frame = nullptr;
    // render scale (vxpt_upscale): the upscaled frame (followed by the sharpener's input image when that
    // mode is used), grown on demand; the last call's size and events
    float4 *upscaled = nullptr;
    size_t upscaledCap = 0;
    int upW = 0, upH = 0;
    hipEvent_t upEv[2] = {};
    unsigned *postHist = nullptr;
    float *postState = nullptr;
    float sunLuminance = 1.0f;     // SkyModel::getAccumulatedSunLuminance: the sun map's total pdf

    vxpt_denoise_params yamlDenoise{};
    float skyParams[4] = {0.25f, 45.0f, 0.0f, 1.0f};
    vxpt_material yamlMats[13] = {};

    // band partition (multi-GPU): this context's rank among nranks bands and the
    // transport its halo rows move by -- an RCCL communicator (one process per
    // GPU) or the other contexts of this process (vxpt_band_link)
    int nranks = 1, rank = 0;
    std::vector<int> splits;  // nranks + 1 band boundaries (row_splits, or the equal bands)
    ncclComm_t comm = nullptr;
    std::vector<vxpt_ctx *> linked;
    // the trace-halo exchange runs on its own stream, overlapped with the next
    // pass up to its temporal-reuse kernel (haloDone: recorded after the exchange)
    hipStream_t commStream = nullptr;
    hipEvent_t haloReady = nullptr, haloDone = nullptr;
    // exDone: after the last exchange in stream order; the exchange stream's next group waits for it,
    // and an exchange in stream order waits for an exchange-stream group still pending (haloDone):
    // the communicator's groups run one after another, in the order every rank issues them
    hipEvent_t exDone = nullptr;
    bool exDoneRec = false;
    // vxpt_band_stats collection: timing events from a pool bracketing each exchange group (kind 0 on
    // the context stream, 1 on the exchange stream) and each banded frame's trace (2) and denoiser (3)
    // spans, and the bytes sent to each neighbour.  Completed spans are folded into `ms` and their
    // events reused (stat_fold: at every sync of a banded run, and before a frame once the pool holds
    // kStatPoolFold events), so a long collection keeps a bounded pool.
    struct BandStat {
        bool on = false;
        std::vector<hipEvent_t> pool;
        size_t used = 0;
        struct Span { size_t e0, e1; int kind; };
        std::vector<Span> spans;
        double ms[4] = {};
        int frames = 0, groups = 0, groupsOrdered = 0;
        double up = 0.0, down = 0.0;
    } bst;
    // halo depths the last banded frame exchanged: tap records + reservoirs, histories, G-buffer planes
    int haloTraceRows = 72, haloHistRows = 2, haloPlaneRows = 40;
    bool haloPending = false;
};

#pragma GCC visibility push(hidden)
namespace vx::host {

inline int fail(vxpt_ctx *c, int code, const std::string &msg) {
    if (c) c->err = msg;
    return code;
}
#define HIPCHK(c, expr)                                                                          \
    do {                                                                                         \
        hipError_t e_ = (expr);                                                                  \
        if (e_ != hipSuccess) return fail((c), VXPT_ERR_HIP, std::string(#expr) + ": " + hipGetErrorString(e_)); \
    } while (0)

template <class T>
int dalloc(vxpt_ctx *c, T *&p, size_t n) {
    void *q = nullptr;
    HIPCHK(c, hipMalloc(&q, n * sizeof(T) + 16));
    HIPCHK(c, hipMemsetAsync(q, 0, n * sizeof(T) + 16, c->stream));  // same stream as every upload
    c->allocs.push_back(q);
    p = (T *)q;
    return 0;
}

template <class T>
int grow(vxpt_ctx *c, DBuf<T> &d, size_t n) {
    if (d.n >= n) return 0;
    if (dalloc(c, d.p, n)) return 1;
    d.n = n;
    return 0;
}

// a buffer that a steady edit loop does not reallocate: grown to twice the need
template <class T>
int grow2(vxpt_ctx *c, DBuf<T> &d, size_t n) {
    if (d.n >= n) return 0;
    const size_t cap = std::max(n, 2 * d.n);
    if (dalloc(c, d.p, cap)) return 1;
    d.n = cap;
    return 0;
}

template <class T>
int upload_vec(vxpt_ctx *c, DBuf<T> &d, const T *h, size_t n) {
    if (d.n < n) {
        if (dalloc(c, d.p, n)) return VXPT_ERR_HIP;
        d.n = n;
    }
    HIPCHK(c, hipMemcpyAsync(d.p, h, n * sizeof(T), hipMemcpyHostToDevice, c->stream));
    return 0;
}

// A pass whose first half is enqueued (trace_front) and whose second half is not yet (trace_back).
struct PassPlan {
    TraceArgs a;
    int next = 0, set = 0;
};

constexpr int kWposHalo = 40;  // firefly_band's rows either side of the band (host_frame.cpp)
constexpr int kDenoiseRows = kWposHalo;  // the deepest read of the current G-buffer planes by the denoiser

// the context's denoiser settings for a call that passes none
inline const vxpt_denoise_params *denoise_or_yaml(const vxpt_ctx *c, const vxpt_denoise_params *p) {
    return p ? p : &c->yamlDenoise;
}

// vxpt_host.cpp
CamDev make_camera(int W, int H, const vxpt_camera &in, float *yawOut, float *pitchOut);
CamDev make_camera_src(int W, int H, const vxpt_ctx::CamSrc &s);
CamDev history_camera(const vxpt_ctx *c, const vxpt_ctx::CamSrc &s);
void release_held_camera(vxpt_ctx *c);
bool buffer_ptr(vxpt_ctx *c, int which, void *&p, size_t &bytes, bool forWrite, void **mirror);

// host_settings.cpp
std::string trim(const std::string &s);
std::map<std::string, std::string> parse_flow_map(const std::string &s);
std::vector<float> parse_list(const std::string &s);
bool as_bool(const std::string &s);
vxpt_post_params default_post();
const vxpt_denoise_params &default_denoise();

// host_world.cpp
void box_fill(vxpt_ctx *c, int oct, int x0, int x1, int y0, int y1, int z0, int z1);
void brick_prefix(vxpt_ctx *c);
int device_tables(vxpt_ctx *c);
int world_from_device(vxpt_ctx *c, hipEvent_t tables, hipEvent_t read);
float nearest_surface(const vxpt_ctx *c, V3 p);

// host_sky.cpp
std::vector<AliasBin> build_alias(const std::vector<float> &w, float &sumOut);

// host_instances.cpp
MeshDev mesh_dev(const vxpt_ctx *c);
int edit_instances(vxpt_ctx *c, int x, int y, int z, int old, int block_id);

// host_frame.cpp
void fill_world(vxpt_ctx *c, WorldDev &w);
hipStream_t front_stream(const vxpt_ctx *c, int set);
int trace_front(vxpt_ctx *c, int32_t it, uint32_t flags, bool accumulate, bool accumFirst, float accumScale,
                bool overlap, PassPlan &pl, bool planes = true);
bool chain_gate(const vxpt_ctx *c, int spp);
int trace_back(vxpt_ctx *c, const PassPlan &pl, bool mark = true);
int do_trace(vxpt_ctx *c, int32_t it, uint32_t flags, bool accumulate, bool accumFirst, float accumScale,
             bool overlap = false, bool mark = true, bool planes = true);
const char *prefilter_switch(const vxpt_denoise_params *p);
int refuse_prefilter(vxpt_ctx *c, const char *sw);
bool is_banded(const vxpt_ctx *c);
int do_denoise(vxpt_ctx *c, const vxpt_denoise_params *p, int frameNum, int it);
int run_pass(vxpt_ctx *c, const vxpt_denoise_params *p, int pass, int arg, int arg2, int margin = 0);

// host_bands.cpp
void gbuf_written(vxpt_ctx *c, int which);
int stat_sync_fold(vxpt_ctx *c);
void band_timings(std::vector<vxpt_ctx *> &cs);
int band_frame(std::vector<vxpt_ctx *> &cs, const vxpt_denoise_params *p, int frame, int spp, bool sync = true,
               std::vector<PassPlan> *pipe = nullptr, bool pipeNext = false);

}  // namespace vx::host
#pragma GCC visibility pop

// Dynamic symbols of the library beside include/vxpt.h's (and tuning_defaults above), by name: the parent exported them, and the
// exported surface does not change with the files.  They keep their linkage and visibility.
extern "C" {
int refresh_instances(vxpt_ctx *c, bool lights, bool full);  // instanced meshes (+ lights), after the grid changed
int refresh_instances_edit(vxpt_ctx *c, bool lights, bool full, const int *edit);  // the same after one edit
int inst_flush(vxpt_ctx *c);     // what a batch of edits left to enqueue (device instance mode)
int alias_scratch(vxpt_ctx *c, int n);  // the alias kernels' scratch: the sky's and the light tables' builds share it
int sky_resolve(vxpt_ctx *c);    // the sun table's sum and the build time of a device sky build
int post_alloc(vxpt_ctx *c);
int post_args(vxpt_ctx *c, const vxpt_post_params *pp, float dtMs, PostArgs &a);
int band_post(std::vector<vxpt_ctx *> &cs, const vxpt_post_params *pp, float dtMs);
}
