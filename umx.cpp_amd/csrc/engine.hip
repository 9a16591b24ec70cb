// engine.hip -- C-ABI implementation (include/umx_hip.h) of the gfx950 UMX segment engine.
// Orchestrates one segment exactly like umx_inference (inference.cpp:12-207):
//   stft -> |.| / crop+stack -> 4 x [fc1 bn tanh -> 3-layer BiLSTM -> fc2 bn relu -> fc3 bn scale
//   relu -> mask*mix] -> Wiener EM -> 4 x istft
// The four targets run inside the same launches; consecutive segments alternate between two pipeline
// slots (streams) so that their LSTM layers overlap as an exact wavefront (see struct Slot).  A context created
// for several tracks (umx_hip_create_tracks) runs one segment of each track per call: every stage is queued for
// all track lanes, and the LSTM recurrence of all lanes is ONE launch (lstm_batch.h).  Also here: the
// whole-track drivers (split / shift inference with the track resident in HBM), the phased form of a segment
// for the multi-GPU state-carry mode, weight residency (u8/u16 as stored, or expanded) and the GEMM flavour.
#include "../../include/umx_hip.h"
#include <chrono>
#include <dlfcn.h>

#include <algorithm>
#include <numeric>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <mutex>
#include <string>
#include <vector>

#include "common.h"
#include "gemm_bf16x3.h"
#include "gemm_planes.h"
#include "gemm_planes_pp.h"
#include "gemm_planes_ps.h"
#include "lstm_kernels.h"
#include "lstm_batch.h"
#include "lstm_batch8.h"
#include "track_kernels.h"
#include "resample.h"
#include "stft_kernels.h"
#include "wiener_kernels.h"
#include "wiener_istft.h"
#include "wiener_em.h"
#include "residual_mask.h"
#include "softmask.h"
#include "shift_mean.h"
#include "stem_mix.h"
#include "sample_format.h"
#include "pcm16.h"
#include "pcm24.h"
#include "levels.h"
#include "loudness.h"
#include "true_peak.h"
#include "gate_debug.h"

using namespace umx;

// UMX_HIP_CHECK for the free functions of the C-ABI (the error goes to the context)
#define UMX_HIP_CHECK_CTX(ctx_, expr)                                                                                \
    do                                                                                                               \
    {                                                                                                                \
        hipError_t _e = (expr);                                                                                      \
        if (_e != hipSuccess)                                                                                        \
        {                                                                                                            \
            (ctx_)->set_error(std::string(#expr) + ": " + hipGetErrorString(_e));                                    \
            return UMX_ERR_HIP;                                                                                      \
        }                                                                                                            \
    } while (0)

namespace
{
std::string g_create_error = "";

// The weights of the dense stack, one per GEMM stage: fc1, W_ih of layers 0-2, fc2, fc3.
enum { W_FC1 = 0, W_IH0, W_IH1, W_IH2, W_FC2, W_FC3, W_COUNT };
inline int gemm_weight(int mode, int layer) { return mode == G_FC1 ? W_FC1 : mode == G_IH ? W_IH0 + layer : mode == G_FC2 ? W_FC2 : W_FC3; }

// One GEMM weight in HBM, [N][K] per plane.  Plane flavour (gemm_planes.h): `form` fp16 planes -- u8 as 1 exact plane of q - c,
// u16 as 2 planes whose sum is exactly q - c (fp16(q - c) and the remainder, an integer of at most 16), c each source tensor's own
// centre (quant_planes.h), fp32 as 2 split terms of w / s with s a power of two; (s, o) = (scale, offset + c scale), or (s, 0).  Staged flavour (gemm_bf16x3.h): `form` is
// the GemmBType -- BQ_U8 / BQ_U16 = the ggml file's bytes (BASELINE config 5) with (scale, offset) and, for the u8 one-plane form,
// (c, o2) = (the tensor's centre, offset + c scale: quant_centre, quant_planes.h); BQ_F32 = three bf16 planes with (1, 0).  Two of
// each because W_ih of a layer is two file tensors (forward rows, then reverse rows).
struct GemmWeight
{
    const void *p = nullptr;
    int form = 0;
    float s[2] = {1.f, 1.f}, o[2] = {0.f, 0.f};
    float c[2] = {128.f, 128.f}, o2[2] = {0.f, 0.f};
};

struct TargetBufs // weights of one target (shared by both pipeline slots)
{
    GemmWeight w[W_COUNT];
    float *in_scale = nullptr, *in_mean = nullptr, *bn1[4] = {};
    float *ih_b[3] = {};
    float *bn2[4] = {};
    float *bn3[4] = {}, *out_scale = nullptr, *out_mean = nullptr;
};

struct TargetAct // activations of one target in one pipeline slot
{
    float *cat = nullptr, *la = nullptr, *lb = nullptr, *P = nullptr, *a2 = nullptr,
          *mag = nullptr; // mag: fc3's MASK [2][T][MAGP]; x |X| = the target magnitude, formed by the consumers (gemm_common.h)
    // gemm_planes.h: every GEMM's A operand split once into two fp16 planes of the scaled row, its row sums and (for the
    // unbounded tensors) its per-row inverse scales
    unsigned short *xs_p = nullptr, *cat_p = nullptr, *la_p = nullptr, *lb_p = nullptr, *a2_p = nullptr;
    float *rs_xs = nullptr, *rs_catL = nullptr, *rs_catR = nullptr, *rs_la = nullptr, *rs_lb = nullptr, *rs_a2 = nullptr;
    float *rsc_xs = nullptr, *rsc_a2 = nullptr;
};

enum
{
    ST_STFT = 0,
    ST_FC1,
    ST_IH0,
    ST_LSTM0,
    ST_IH1,
    ST_LSTM1,
    ST_IH2,
    ST_LSTM2,
    ST_FC2,
    ST_FC3,
    ST_WIENER,
    ST_ISTFT,
    ST_OLA,
    ST_COUNT
};
enum { SP_XS = 0, SP_CATL, SP_LA, SP_LB, SP_CATR, SP_A2 }; // which A operand launch_split prepares
const char *kStageNames[ST_COUNT] = {"stft",  "fc1", "lstm_ih0", "lstm_rec0", "lstm_ih1", "lstm_rec1", "lstm_ih2",
                                     "lstm_rec2", "fc2", "fc3_mask", "wiener",  "istft",    "ola"};

// roctx ranges per stage (tracing): every stage marker below also opens a named range on the calling thread
// ("umx:<stage>": the HOST span in which the stage's kernels are queued; rocprofv3 --marker-trace shows them beside the
// kernel trace).  The marker library is used only if a profiler has ALREADY loaded it into the process (RTLD_NOLOAD) or
// UMX_ROCTX=1 asks for it: an installed ROCm alone does not make every stage marker a library call on the queuing path.
namespace
{
struct RoctxApi
{
    int (*push)(const char *) = nullptr;
    int (*pop)() = nullptr;
    char names[ST_COUNT][40];
    RoctxApi()
    {
        for (int i = 0; i < ST_COUNT; ++i)
            snprintf(names[i], sizeof names[i], "umx:%s", kStageNames[i]);
        const char *want = getenv("UMX_ROCTX");
        const bool force = want && atoi(want) != 0;
        for (const char *lib : {"librocprofiler-sdk-roctx.so", "libroctx64.so"})
            if (void *h = dlopen(lib, force ? (RTLD_NOW | RTLD_LOCAL) : (RTLD_NOW | RTLD_NOLOAD)))
            {
                push = reinterpret_cast<int (*)(const char *)>(dlsym(h, "roctxRangePushA"));
                pop = reinterpret_cast<int (*)()>(dlsym(h, "roctxRangePop"));
                if (push && pop)
                    return;
                push = nullptr;
                pop = nullptr;
            }
    }
};
thread_local bool t_stage_range_open = false;
// closes the calling thread's open stage range and opens `stage` (< 0: only closes; every exit of a call, error returns and
// umx_hip_segment_discard included, ends with stage_range(-1))
inline void stage_range(int stage)
{
    static const RoctxApi api;
    if (!api.push)
        return;
    if (t_stage_range_open)
        api.pop();
    t_stage_range_open = stage >= 0 && stage < ST_COUNT;
    if (t_stage_range_open)
        api.push(api.names[stage]);
}
struct StageRangeCloser // closes whatever stage range is open when a queuing function returns, on every path
{
    ~StageRangeCloser() { stage_range(-1); }
};
} // namespace

// One track lane of a pipeline slot = the activations of one in-flight segment of one track.
struct Lane
{
    TargetAct ta[4];
    float2 *spec = nullptr, *y = nullptr, *frames = nullptr;
    float *x = nullptr, *wpart = nullptr, *Rc = nullptr;
    unsigned *maxabs = nullptr;
};

// One pipeline slot = everything one in-flight segment (of every track lane) needs.  Two slots on two streams let
// segment s+1 run its STFT/GEMMs and LSTM layer l while segment s is in layer l+1 (the exact wavefront of
// R_l(s+1) waits only for R_l(s) through an event); the single-track LSTM kernels are latency-bound
// and use half of each CU's wave slots, so two of them co-reside and fill each other's hand-off gaps.
struct Slot
{
    hipStream_t stream = nullptr;
    Lane lane[LSTMB_MAX_TRACKS];
    float *hbuf = nullptr;
    float *wv = nullptr; // Wiener EM state v [T][2049][4] of every lane (wiener_em.h): allocated by the first call that asks for 2+ iterations
    bool lstm_wrote_planes[3] = {false, false, false}; // this call's recurrence of layer l wrote the next GEMM's A planes (run_lstm_layer_batched)
    bool lstm_rows_f32[3] = {true, true, true};        // ... and its fp32 output rows as well (else only the launch's last row: the taps of that layer are unavailable)
    unsigned *status = nullptr, *lsync = nullptr;
    unsigned long long *lprof = nullptr;
    hipEvent_t ev[ST_COUNT + 1] = {};
    hipEvent_t evk[ST_COUNT] = {}; // GEMM stages of plane contexts: recorded between the stage's split kernel and its GEMM kernel
    bool evk_set[ST_COUNT] = {};
    hipEvent_t rec_done[3] = {}; // LSTM layer l of this slot's segment has finished (state updated)
    // host-pointer entry points (see umx_hip_infer_batch_async): the download of call k's stems is queued on the OTHER slot's
    // stream, behind call k + 1's kernels
    hipEvent_t k_done = nullptr;   // this slot's stems are complete (recorded on its own stream)
    hipEvent_t out_free = nullptr; // their download has finished (recorded on the other slot's stream): overlap-add may overwrite them
    bool out_free_valid = false;
    bool have_times = false, last_persistent = false, used = false;
};
} // namespace

// Admission of persistent LSTM grids, process-wide and per device.  A persistent launch needs ALL its workgroups
// co-resident (they exchange granules), so the grids that can be resident TOGETHER must fit the device together.
// Grids queued on one stream run one after the other, so a stream contributes at most its largest queued grid; what has
// to fit is the sum over streams.  A launch that would not fit is made to wait -- on the device, through a stream-wait
// on another stream's newest admitted grid (which, streams being in order, is a wait for all of that stream's grids),
// never by blocking the host -- for the streams whose queued grids are oldest, until it fits.  The streams it waits for
// hold only grids admitted earlier, i.e. work that does not depend on the new launch: no cycle.
// (Rounds 1-2 summed over all queued grids instead of over streams: with the host running ahead of the device, a launch then
// waited for every earlier grid but the most recent one, and the two-slot wavefront of a single-track context overlapped
// only L2(s) with L0(s+1) -- one pair per segment instead of every layer.  Found in round 3.)
// Units are half CUs: a single-track workgroup (two fit a CU) counts 1, a batched one (one per CU) counts 2.
namespace
{
struct LstmGate
{
    std::mutex m;
    struct Grid
    {
        hipEvent_t done;
        int units;
        hipStream_t stream;
        unsigned long long seq;
    };
    std::vector<Grid> inflight; // in admission order
    std::vector<hipEvent_t> pool;
    unsigned long long seq = 0;
    int reserved = 0; // half CUs kept free for kernels that are not this engine's (RCCL send / recv: umx_hip_gate_reserve)
    std::vector<int> reservations; // outstanding requests in CUs: `reserved` is twice their sum
};
LstmGate g_gate[16];

// admit + launch + record under the gate's lock (an event that has not been recorded yet would read as complete)
template <class Launch> hipError_t lstm_gate_launch(int device, hipStream_t st, int units, int capacity_units, Launch launch)
{
    LstmGate &g = g_gate[device & 15];
    std::lock_guard<std::mutex> lock(g.m);
    capacity_units -= std::min(g.reserved, capacity_units / 2);
    for (size_t i = 0; i < g.inflight.size();)
        if (hipEventQuery(g.inflight[i].done) == hipSuccess)
        {
            g.pool.push_back(g.inflight[i].done);
            g.inflight.erase(g.inflight.begin() + i);
        }
        else
            ++i;
    (void)hipGetLastError(); // hipEventQuery reports "not ready" as an error
    // per other stream: its largest queued grid, the admission number of its oldest one, and its newest grid's event
    struct PerStream
    {
        hipStream_t stream;
        int units;
        unsigned long long oldest;
        hipEvent_t newest;
    };
    std::vector<PerStream> others;
    for (const LstmGate::Grid &gr : g.inflight)
    {
        if (gr.stream == st)
            continue;
        PerStream *ps = nullptr;
        for (PerStream &o : others)
            if (o.stream == gr.stream)
                ps = &o;
        if (!ps)
        {
            others.push_back({gr.stream, 0, gr.seq, gr.done});
            ps = &others.back();
        }
        ps->units = std::max(ps->units, gr.units);
        ps->newest = gr.done; // admission order: the last one seen is the newest
    }
    int used = 0;
    for (const PerStream &o : others)
        used += o.units;
    while (used + units > capacity_units && !others.empty())
    {
        size_t k = 0;
        for (size_t i = 1; i < others.size(); ++i)
            if (others[i].oldest < others[k].oldest)
                k = i;
        (void)hipStreamWaitEvent(st, others[k].newest, 0); // every grid of that stream has left the device when we start
        used -= others[k].units;
        others.erase(others.begin() + k);
    }
    hipEvent_t ev = nullptr;
    if (!g.pool.empty())
    {
        ev = g.pool.back();
        g.pool.pop_back();
    }
    else if (hipEventCreateWithFlags(&ev, hipEventDisableTiming) != hipSuccess)
        ev = nullptr;
    const hipError_t e = launch();
    if (ev && e == hipSuccess && hipEventRecord(ev, st) == hipSuccess)
        g.inflight.push_back({ev, units, st, g.seq++});
    else if (ev)
        g.pool.push_back(ev);
    return e;
}
} // namespace

template <class K> static const void *kernel_ptr(K *k) { return reinterpret_cast<const void *>(k); }

#ifndef UMX_FUSE_LSTM_PLANES
#define UMX_FUSE_LSTM_PLANES 1
#endif
// The LSTM kernel table: (family, LSTM hidden size Hl, W_hh u8-resident, PRECISE activations, octets per workgroup) -> kernel and
// the dynamic LDS its limit is raised to.  It holds the only instantiations of the three recurrences; init walks it for the LDS
// limits and the occupancy, the launches take their kernel from here.
//   lstm_persistent_kernel  one track; fp32- and u8-resident W_hh in one kernel (u8 = -1)
//   lstm_batch_kernel       a group of 16 lanes per launch; lds = the 16-lane worst case (a launch passes what its lanes need)
//   lstm_batch8_kernel      octets of 8 lanes x column shards of 64 units (lstm_batch8.h): Hl 512 (UMX-L) and 256 (umxhq),
//                           u8-resident W_hh only; two octets per workgroup in turn: hidden 1024, 33 .. 64 lanes in one launch;
//                           dbg = 1: lstm_batch8_dbg_kernel, the same with the phase profiler and the abort test (the launches that ask for either)
enum { LSTM_PERSISTENT = 0, LSTM_BATCH, LSTM_BATCH8 };
struct LstmKernel
{
    int family, hl, u8, precise, octets;
    const void *fn;
    size_t lds;
    int dbg = 0;
};
#define LSTM_ROW_P(HL, PR) {LSTM_PERSISTENT, HL, -1, PR, 1, kernel_ptr(lstm_persistent_kernel<HL / 8, PR>), 0}
#define LSTM_ROW_B(HL, U8, PR) {LSTM_BATCH, HL, U8, PR, 1, kernel_ptr(lstm_batch_kernel<HL, U8, PR>), lstmb_lds_bytes(LSTMB_GROUP_TRACKS, lstmb_lanes(LSTMB_GROUP_TRACKS).bulk)}
#define LSTM_ROW_8(HL, PR, NO) {LSTM_BATCH8, HL, 1, PR, NO, kernel_ptr(lstm_batch8_kernel<HL, PR, NO>), lstm8_lds_bytes(HL, NO)}, \
                               {LSTM_BATCH8, HL, 1, PR, NO, kernel_ptr(lstm_batch8_dbg_kernel<HL, PR, NO>), lstm8_lds_bytes(HL, NO), 1}
#define LSTM_ROWS_P(HL) LSTM_ROW_P(HL, false), LSTM_ROW_P(HL, true)
#define LSTM_ROWS_B(HL) LSTM_ROW_B(HL, false, false), LSTM_ROW_B(HL, false, true), LSTM_ROW_B(HL, true, false), LSTM_ROW_B(HL, true, true)
#define LSTM_ROWS_8(HL) LSTM_ROW_8(HL, false, 1), LSTM_ROW_8(HL, true, 1), LSTM_ROW_8(HL, false, 2), LSTM_ROW_8(HL, true, 2)
static const LstmKernel kLstmKernels[] = {
    LSTM_ROWS_P(64), LSTM_ROWS_P(128), LSTM_ROWS_P(256), LSTM_ROWS_P(512), //
    LSTM_ROWS_B(64), LSTM_ROWS_B(128), LSTM_ROWS_B(256), LSTM_ROWS_B(512), //
    LSTM_ROWS_8(256), LSTM_ROWS_8(512),
};
#undef LSTM_ROWS_8
#undef LSTM_ROWS_B
#undef LSTM_ROWS_P
#undef LSTM_ROW_8
#undef LSTM_ROW_B
#undef LSTM_ROW_P
static const LstmKernel *lstm_kernel(int family, int hl, bool u8, bool precise, int octets = 1, bool dbg = false)
{
    for (const LstmKernel &k : kLstmKernels)
        if (k.family == family && k.hl == hl && (k.u8 < 0 || k.u8 == (int)u8) && k.precise == (int)precise && k.octets == octets && k.dbg == (int)dbg)
            return &k;
    return nullptr;
}
// "{128, 256, ...}": the hidden_size values (2 Hl) a family has kernels for
static std::string lstm_hidden_sizes(int family)
{
    std::string s;
    int last = 0;
    for (const LstmKernel &k : kLstmKernels)
        if (k.family == family && k.hl != last)
        {
            s += (s.empty() ? "{" : ", ") + std::to_string(2 * k.hl);
            last = k.hl;
        }
    return s + "}";
}

// The GEMM kernel tables: (stage, form of the weight[, tile kind]) -> kernel and its dynamic LDS.  They hold the only
// instantiations of the GEMM kernels; init raises the LDS limit of every entry and the launches take theirs from here.  The
// u8 weights (fc1, W_ih) come in every form, the u16 ones (fc2, fc3) only as two planes (plane flavour) or as u16 / fp32 (staged).
struct GemmKernel
{
    const void *fn = nullptr;
    int lds = 0;
};

// gemm_bf16x3_kernel by GemmBType
template <int MODE> static GemmKernel bx_kernel_m(int bq)
{
    if (bq == BQ_F32)
        return {kernel_ptr(gemm_bf16x3_kernel<MODE, BQ_F32>), BX_LDS_BYTES};
    if constexpr (MODE == G_FC1 || MODE == G_IH)
    {
        if (bq == BQ_U8X)
            return {kernel_ptr(gemm_bf16x3_kernel<MODE, BQ_U8X>), BX_LDS_BYTES};
        if (bq == BQ_U8)
            return {kernel_ptr(gemm_bf16x3_kernel<MODE, BQ_U8>), BX_LDS_BYTES};
    }
    else if (bq == BQ_U16)
        return {kernel_ptr(gemm_bf16x3_kernel<MODE, BQ_U16>), BX_LDS_BYTES};
    return {};
}
static GemmKernel bx_kernel(int mode, int bq)
{
    switch (mode)
    {
    case G_FC1: return bx_kernel_m<G_FC1>(bq);
    case G_IH: return bx_kernel_m<G_IH>(bq);
    case G_FC2: return bx_kernel_m<G_FC2>(bq);
    default: return bx_kernel_m<G_FC3>(bq);
    }
}

// the plane GEMMs by planes of B and tile kind: lock step with 128 x 128 or 256 x 256 tiles (gemm_planes.h), 256 x 256 in
// ping-pong (gemm_planes_pp.h) or persistent (gemm_planes_ps.h)
enum { GP_128 = 0, GP_256, GP_PP, GP_PS, GP_KINDS };
template <int MODE, int NBP> static GemmKernel gp_kernel_mn(int kind)
{
    switch (kind)
    {
    case GP_128: return {kernel_ptr(gemm_planes_kernel<MODE, NBP, 2, 2>), gp_lds_bytes(2, 2, NBP)};
    case GP_256: return {kernel_ptr(gemm_planes_kernel<MODE, NBP, 4, 4>), gp_lds_bytes(4, 4, NBP)};
    case GP_PP: return {kernel_ptr(gemm_planes_pp_kernel<MODE, NBP>), gp_lds_bytes(4, 4, NBP)};
    default: return {kernel_ptr(gemm_planes_ps_kernel<MODE, NBP>), ps_lds_bytes(NBP)};
    }
}
template <int MODE> static GemmKernel gp_kernel_m(int nbp, int kind)
{
    if constexpr (MODE == G_FC1 || MODE == G_IH)
    {
        if (nbp == 1)
            return gp_kernel_mn<MODE, 1>(kind);
    }
    return nbp == 2 ? gp_kernel_mn<MODE, 2>(kind) : GemmKernel{};
}
static GemmKernel gp_kernel(int mode, int nbp, int kind)
{
    switch (mode)
    {
    case G_FC1: return gp_kernel_m<G_FC1>(nbp, kind);
    case G_IH: return gp_kernel_m<G_IH>(nbp, kind);
    case G_FC2: return gp_kernel_m<G_FC2>(nbp, kind);
    default: return gp_kernel_m<G_FC3>(nbp, kind);
    }
}

struct umx_hip_ctx
{
    int device = 0, H = 0, Hl = 0, S = 0, N = 0, T = 0, Tp = 0, nbatch = 0;
    static constexpr int Mpad = 256; // slack rows behind the last lane: a launch's M is rounded up to the 256-row tile
    std::string err;
    std::vector<void *> allocs;
    TargetBufs tb[4];
    float *whh[3] = {}, *bhh[3] = {};
    float *window = nullptr, *nw = nullptr;
    float2 *tw1 = nullptr, *tw2 = nullptr;
    float *tap_tmp = nullptr;                    // umx_hip_read_tap: scratch of the computed taps
    float *audio_in = nullptr, *out_dev[4] = {}; // device staging of the phased (multi-GPU carry) entry points
    static constexpr int kMaxSlots = 3;
    float *stage_in[kMaxSlots] = {}, *stage_out[kMaxSlots][4 * LSTMB_MAX_TRACKS] = {}; // per pipeline slot: device staging of the host-pointer
    int ensure_staging();                                              // entry points, [lane] / [lane][4]; allocated on first use
    hipEvent_t order_ev = nullptr;
    struct DeferredDownload // the stems of a host-pointer call, in its slot's staging buffers
    {
        bool valid = false;
        int si = 0, nb = 0, n[LSTMB_MAX_TRACKS] = {};
        float *host[4 * LSTMB_MAX_TRACKS] = {};
    };
    int queue_download(const DeferredDownload &d, hipStream_t on); // D2H copies of d onto stream `on`, then out_free of its slot
    hipStream_t copy_stream = nullptr; // downloads of the host-pointer calls (created with the staging buffers)
    float *state = nullptr, *state_alt = nullptr; // state_alt: second copy for the per-step driver of the batched recurrence
    Slot slot[kMaxSlots];
    int nslots = 2; // pipeline slots: 3 for single-track contexts (see init), 2 for track-batched ones
    int next_slot() const { return (int)(nseg % nslots); }
    void clear_used()
    {
        for (int si = 0; si < kMaxSlots; ++si)
            slot[si].used = false;
    }
    int B = 1;                // track lanes (umx_hip_create_tracks); every lane has its own streaming LSTM state
    bool lstm_batched = false; // LSTM recurrence on the matrix cores for all lanes at once (lstm_batch.h); fixed at
                               // create so that a track's bits never depend on how many lanes a call uses
    unsigned tag_epoch = 0;   // persistent LSTM launches so far (granule tags are unique per launch)
    unsigned next_tag_base()
    {
        // 4096 tags per launch (T + 1 <= 4096 is checked at create); wraps after ~1M launches, where one
        // stale line from exactly 2^20 launches ago would have to survive in an L2 -- every buffer is
        // zeroed at that point anyway (see run_lstm_layer)
        tag_epoch = (tag_epoch + 1) & 0xFFFFF;
        return tag_epoch << 12;
    }
    int cur = 0;              // slot of the most recently queued segment
    long long nseg = 0;       // segments queued since creation
    size_t lsync_words = 0;
    bool persistent_ok = true;
    int n_cus = 256;
    // what umx_hip_sync needs to redo the calls queued since the last sync after a persistent-kernel timeout
    struct PendingCall
    {
        int nb;
        const float *audio[LSTMB_MAX_TRACKS];
        int n[LSTMB_MAX_TRACKS];
        float *out[4 * LSTMB_MAX_TRACKS];
        float *host_out[4 * LSTMB_MAX_TRACKS]; // host-pointer entry points: where the stems are copied afterwards
        const float *host_audio[LSTMB_MAX_TRACKS]; // ... and where the audio came from: the two staging buffers have been
                                                   // reused by later calls, so a replay uploads it again
        unsigned flags;
    };
    static constexpr int kBackupCalls = 8;
    std::vector<PendingCall> pending; // at most kBackupCalls entries
    bool pending_lost = false;        // calls were queued that cannot be replayed: more than kBackupCalls since the last sync,
                                      // or the caller was released from the buffer contract (umx_hip_order_before)
    float *backup = nullptr; // [kBackupCalls][3 layers][B * state_floats]: the stream state right before each layer launch
    bool no_recovery = false, recovering = false;
    int recover();
    int lstm_poll_delay = 0;         // 0 = the kernel's default (LSTM_POLL_DELAY)
    int env_gemm_ps = -1;            // UMX_GEMM_PS: bit per GemmMode, which 256 x 256 launches take the persistent kernel (gemm_planes_ps.h); < 0: all
    int env_gemm_pp = -1;            // UMX_GEMM_PP: bit mask of the GEMMs that take the ping-pong kernel; < 0: all.  Both are read ONCE, when the context is created: a test makes a context per mode
    const char *gemm_kernel_last[4] = {"none", "none", "none", "none"}; // per GemmMode (umx_hip_gemm_kernel_name)
    const char *lstm_kernel_last = "none"; // the recurrence kernel of the last layer launch (umx_hip_lstm_kernel_name)
    int lstm_capacity = 0;           // workgroups of the persistent LSTM kernel that can be co-resident
    unsigned last_flags = 0;
    hipStream_t stream = nullptr; // = slot[0].stream (H2D/D2H of the host-pointer entry point)

    void set_error(const std::string &s) { err = s; }

    template <class T_> int dalloc(T_ **p, size_t count, bool zero = true)
    {
        void *q = nullptr;
        UMX_HIP_CHECK(hipMalloc(&q, std::max<size_t>(count, 1) * sizeof(T_)));
        allocs.push_back(q);
        if (zero)
            UMX_HIP_CHECK(hipMemset(q, 0, std::max<size_t>(count, 1) * sizeof(T_)));
        *p = reinterpret_cast<T_ *>(q);
        return UMX_OK;
    }
    // the release that goes with dalloc: p leaves `allocs` and the device, and is nulled; a pointer dalloc did not hand out is an error
    template <class T_> int dfree(T_ *&p)
    {
        const auto it = std::find(allocs.begin(), allocs.end(), (void *)p);
        if (it == allocs.end())
        {
            set_error("dfree: not a device buffer of this context");
            return UMX_ERR_HIP;
        }
        allocs.erase(it);
        (void)hipFree(p);
        p = nullptr;
        return UMX_OK;
    }
    // Grow-only device buffers (engine_tracks.h): every pointer of `bufs` has room for (its elements per unit) x `units`; `cap`: the
    // units they hold now.  Too small: all are released and allocated again with an eighth to spare (their contents are lost).
    template <class T_> int grow_only(std::initializer_list<std::pair<T_ **, int>> bufs, size_t &cap, size_t units);
    template <class T_> int upload(T_ **p, const std::vector<T_> &h)
    {
        int rc = dalloc(p, h.size(), false);
        if (rc)
            return rc;
        UMX_HIP_CHECK(hipMemcpy(*p, h.data(), h.size() * sizeof(T_), hipMemcpyHostToDevice));
        return UMX_OK;
    }
    int init(int device_, int hidden, int segment_samples, const umx_tensor_view *tensors, int n_tensors,
             unsigned create_flags, int n_tracks);
    size_t weight_bytes = 0;      // HBM held by model tensors (the config-5 figure of merit)
    bool wiener_fused = true;     // wiener_istft.h: gains + filter + inverse STFT frame in one kernel
    bool gemm_planes = false;     // dense stack with both operands pre-split as fp16 planes and LDS-DMA staging (gemm_planes.h);
                                  // else the three-term bf16 split staged per tile (gemm_bf16x3.h)
    void launch_split(Lane &ln, int nl, hipStream_t st, int which, const int *active, int nact);
    void launch_gemm_planes(Lane &ln, int nl, hipStream_t st, int mode, int layer, const int *active, int nact, bool dbg);
    // one GEMM stage for the track lanes with audio: the plane GEMMs take every run of consecutive lanes in one launch
    void launch_gemm_lanes(Slot &sl, hipStream_t st, int nb, const float *const *audio_dev, int mode, int layer, const int *active,
                           int nact, bool dbg);
    bool u8_dequant = false;      // UMX_CREATE_U8_DEQUANT: u8 weights dequantised per element (model.cpp:610-616) before they
                                  // are multiplied, instead of exact bf16 integers with the affine map applied to the sum
    unsigned char *whh_q[3] = {}; // u8-resident W_hh (create flag), same layout as whh[]
    float whh_s[3][8] = {}, whh_o[3][8] = {};
    int infer_device(const float *audio_dev, int n, float *const out[4], unsigned flags);
    // one segment of each of `nb` track lanes (lane i = track i of this context; audio[i] == nullptr: lane idle)
    int infer_batch(int nb, const float *const *audio_dev, const int *n, float *const *out /* [nb][4] */, unsigned flags);
    int lstm_batch_capacity = 0; // co-resident workgroups of the batched LSTM kernel
    bool lstm_batch8_ok = false; // lstm_batch8_kernel (octets of 8 lanes, lstm_batch8.h) serves this context's batched launches
    int lstm8_poll_delay = 0;    // UMX_LSTM8_POLL_DELAY (read at create)
    bool env_lstm8_paired = true; // UMX_LSTM8_PAIRED=0 (read at create): 33 .. 64 lanes as two launches of 32 instead of two octets per workgroup in turn
    int env_lstm8_min = 1;       // UMX_LSTM8_MIN_LANES (read at create): contexts of at least this many lanes use it (99: none)
    bool lstm_rowsums = false;       // the batched recurrence hands the consuming plane GEMM the row sums of its output (lstm_batch.h, LstmBArgs::rs_dir)
    bool lstm_writes_planes = false; // ... and writes that GEMM's A planes itself
    size_t state_floats() const { return (size_t)4 * 12 * Hl; }
    // phased form of one segment (exact multi-GPU carry): front | layer 0 | layer 1 | layer 2 | back
    // whole tracks on the device (split_inference / shift_inference, umx.cpp:99-295; engine_tracks.h, engine_queue.h)
    // What a whole-track call may ask for beyond its tracks: ONE record, filled by the C entry points (engine_cabi.h), carried by
    // the request of tracks() and by queue(), and kept by every job (admit_job).  Its defaults are the plain call.
    struct TrackOptions
    {
        const MixSpec *mix = nullptr;   // stem_mix.h, DESIGN 17: a checked matrix; weighted sums of a track's stems and its input instead of the stems
        umx_sample_io io = {};          // pcm16.h, DESIGN 19: how the host audio and outputs are read (UMX_SAMPLE_S16: int16 frames behind the float pointers)
        int clip_mode = UMX_CLIP_CLAMP; // levels.h, DESIGN 20: UMX_CLIP_RESCALE: every track leaves whole, over its common divisor
        bool levels = false;            // the caller wants the record of what left
        bool loudness = false;          // loudness.h, DESIGN 21: the hop energies of what leaves are measured
        int true_peak = UMX_TRUE_PEAK_OFF; // true_peak.h, DESIGN 26: MEASURE: the true peak of what leaves is measured; RESCALE: and the divisor comes from it
        bool true_peak_record = false;  // the caller wants the true-peak record
        int n_host() const { return mix ? mix->n_out : 4; } // host buffers per track
        bool rescale() const { return clip_mode == UMX_CLIP_RESCALE; }
        bool measures() const { return levels || rescale(); } // a rescaled track measures for its divisor whether or not the caller wants the record
        bool true_peak_rescale() const { return true_peak == UMX_TRUE_PEAK_RESCALE && rescale(); }
        bool measures_true_peak() const { return true_peak != UMX_TRUE_PEAK_OFF; }
        // a finished span goes through track_leave: something is measured or encoded on its way out
        bool leaves_measured() const { return io.out_format != UMX_SAMPLE_F32 || measures() || loudness || measures_true_peak(); }
    };
    struct TrackRequest // what tracks() is asked for: n_tracks tracks, one per track lane
    {
        int n_tracks = 0;
        const float *const *audio = nullptr;
        const int *length = nullptr;
        const int *rate = nullptr; // nullptr: every track at 44.1 kHz; else track i is at rate[i], resampled to 44.1 kHz and back on the device
        const int *shift_offset = nullptr; // < 0: no shift buffer (plain split_inference)
        float *const *out = nullptr; // opt.n_host() host buffers per track: out[n_host * track + m]
        unsigned flags = 0;
        void (*progress)(float, void *) = nullptr;
        void *progress_user = nullptr;
        bool ensemble = false;       // the lanes are ONE track at n_tracks shift offsets, `out` the buffers of their mean
        TrackOptions opt;            // (opt.levels, opt.loudness, opt.true_peak_record: whether the results below are wanted -- track_request, engine_cabi.h)
        umx_levels *levels = nullptr; // n_tracks records of what left, or nullptr: not wanted
        umx_loudness *loudness = nullptr; // loudness.h, DESIGN 21: n_tracks records, or nullptr
        double *const *hop_energy = nullptr; // per track nullptr or room for its hop energies; either of the two: the tracks are measured
        umx_true_peak *true_peak = nullptr; // true_peak.h, DESIGN 26: n_tracks records, or nullptr (opt.true_peak says whether the tracks are measured)
    };
    int tracks(const TrackRequest &rq);
    int tracks_once(const TrackRequest &rq);
    // resampling (resample.h): the tap table of each (rate_in, rate_out) pair, built once and kept in HBM
    std::map<std::pair<int, int>, float *> rs_taps;
    int resample_plan(int rate_in, int rate_out, ResampleGeom &g, const float **taps_dev);
    struct RsStage // per accumulator set, only once a resampled job borrows it: the track and its outputs at the caller's rate (grow-only)
    {
        float *in = nullptr, *out[4] = {};
        size_t cap = 0; // frames
    };
    int rs_launches[2] = {-1, -1}; // resampler launches (forward, backward) of the last whole-track call or queue run (umx_hip_debug_resample_launches)
    struct TrackBufs // whole-track driver, per track lane: the (shifted) track, 4 stem accumulators, weight sum, 2 x 4 segment stems
    {
        float *in = nullptr, *out[4] = {}, *sumw = nullptr, *seg[kMaxSlots][4] = {};
        size_t cap = 0;
        RsStage rs; // the native-rate staging of a resampled job, frames at the caller's frame numbers
        // DESIGN 19, 24, only once a job asks for UMX_SAMPLE_S16 or UMX_SAMPLE_S24: the track as uploaded and its outputs as they leave, 4
        // or 6 bytes per frame of the CALLER's track (no shift padding; capacities in words), each grow-only on its own
        uint32_t *in_int = nullptr, *out_int[4] = {};
        size_t cap_in_int = 0, cap_out_int[4] = {};
        hipEvent_t in_ev = nullptr; // behind the most recent kernel that wrote `in` -- a decode out of in_int, a resampled range out of rs.in
                                    // (track_upload_until): every call that reads `in` waits for it
        umx_levels_acc *lev = nullptr; // DESIGN 20, only once a job measures: the record of what leaves, zeroed with the accumulators
        double *hopE = nullptr;        // DESIGN 21, only once a job measures loudness: its hop energies [output][channel][hop], grow-only,
        size_t cap_hopE = 0;           // zeroed with the accumulators (cap: doubles)
        unsigned *tp = nullptr;        // DESIGN 26, only once a job measures its true peak: four words, the bit patterns, zeroed with the levels record
    };
    std::vector<TrackBufs> trk;
    hipEvent_t trk_acc_ev[kMaxSlots] = {}; // per slot: behind the overlap-add of the last call that ran in it
    // ---- what tracks_once and the track queue share (engine_tracks.h)
    struct TrackResample // a job at another rate (track_rate_plan): the caller's rate and length, the two rate pairs' geometry and taps
    {
        int rate = 0, length = 0; // rate 0: the job is at 44.1 kHz, nothing below is used
        ResampleGeom fwd, back;   // rate -> 44.1 kHz, 44.1 kHz -> rate
        const float *fwd_taps = nullptr, *back_taps = nullptr;
    };
    int track_rate_plan(int rate, int length_at_rate, const char *too_long, TrackResample &rs, int &n44);
    // The measuring state of a job: the K-weighted hop energies of what leaves go to acc->hopE (opt.loudness), its
    // true peak to acc->tp (opt.true_peak), both over the caller's track as the caller sees it.
    struct TrackMeasure
    {
        int rate = 0;            // the caller's rate: hop = kweight_hop(rate) frames; factor and reach of the interpolator
        long long length = 0;    // frames of the caller's track at that rate
        long long hops = 0;      // whole hops of it
        long long hops_done = 0; // hops already launched
        long long tp_done = 0;   // frames whose true peak is already launched
        void begin(int rate_, long long length_at_rate)
        {
            rate = rate_;
            length = length_at_rate;
            hops = length / kweight_hop(rate);
            restart();
        }
        void restart() { hops_done = tp_done = 0; } // admission, and the queue's restart: what was measured is zeroed and measured again
        size_t hop_doubles(int n_host) const { return std::max<size_t>(1, (size_t)n_host * 2 * (size_t)hops); } // of acc->hopE
    };
    struct TrackJob // a track resident on the device
    {
        const float *audio = nullptr; // on the host (opt.io.in_format UMX_SAMPLE_S16: int16 frames)
        TrackOptions opt;             // what its call asked for (admit_job): mix, the formats of `audio` and of the host buffers its regions
                                      // go to, the clip mode, whether what leaves is measured into acc->lev and acc->hopE
        int length = 0;               // frames as the segments see them (the 44.1 kHz version's of a resampled track)
        int lead = 0, L2 = 0, segs = 0; // track_geometry: frames of silence before the track, padded frames, segments
        long long uploaded = 0;       // host frames already on the device (a resampled job: frames at its own rate, in the set's staging)
        TrackResample rs;             // set before admit_job for a job at another rate; such a job goes in and out by ranges:
        long long done44 = 0;         //   44.1 kHz frames already resampled into the padded signal (even, or `length`)
        long long out_done = 0;       //   frames at the caller's rate already resampled back into the staging (even, or rs.length)
        TrackBufs *acc = nullptr;     // the accumulator set it writes
        bool by_region = true;        // its final regions are mixed in place and leave region by region (false: an ensemble lane, a
                                      // rescaled track -- mixed and downloaded whole behind the last segment)
        bool whole_region = false;    // not by_region, and track_call itself finishes it behind its last segment as ONE region: the
                                      // frames [lead, lead + length) (a rescaled track)
        TrackMeasure m;               // where its loudness and true-peak launches stand (track_measure_grow)
    };
    struct TrackLane // a lane of one call: its job (nullptr: idle) and the padded frame at which its segment starts
    {
        TrackJob *job = nullptr;
        long long start = 0;
    };
    struct TrackRegion // `count` final frames of a job from padded frame `start` on, on the device once `ready` has passed
    {
        TrackJob *job;
        int start, count;
        hipEvent_t ready;
        int rs_first = 0, rs_count = 0; // a resampled job: the frames at the caller's rate that left with it, in the set's staging
    };
    struct TrackRegions // owns the events of its regions: whichever way a driver returns, none is left behind
    {
        std::vector<TrackRegion> v;
        TrackRegions() = default;
        TrackRegions(const TrackRegions &) = delete;
        TrackRegions &operator=(const TrackRegions &) = delete;
        ~TrackRegions() { clear(); }
        void clear()
        {
            for (TrackRegion &r : v)
                if (r.ready)
                    (void)hipEventDestroy(r.ready);
            v.clear();
        }
    };
    struct TrackRun // the scope of a whole-track run: a timeout inside it cannot be repaired call by call (the overlap-add has consumed
    {               // the stems), so umx_hip_sync reports it to the driver; no call of the run stays in the replay log
        umx_hip_ctx &c;
        explicit TrackRun(umx_hip_ctx &c_) : c(c_) { c.no_recovery = true; }
        ~TrackRun()
        {
            c.no_recovery = false;
            c.pending.clear();
            c.pending_lost = false;
        }
    };
    int track_stride() const { return (int)((1 - 0.25f) * N); } // umx.cpp:181, inference.hpp:15
    static bool track_job_ok(const float *audio, int length, int shift_offset, float *const *out, int n_host);
    static bool track_geometry(int length, int shift_offset, int stride, TrackJob &j);
    int track_bufs_grow(TrackBufs &tb_, size_t frames);
    int track_int_grow(TrackBufs &tb_, const umx_sample_io &io, size_t frames, int n_host);
    void track_encode(const TrackBufs &tb_, const umx_sample_io &io, int n_host, float *const src[4], size_t src_start, int count,
                      long long first_frame, umx_levels_acc *acc, hipStream_t st, const uint32_t *words = nullptr);
    int track_measure_grow(TrackBufs &tb_, TrackJob &j, int rate, int length_at_rate);
    struct ZeroSpan
    {
        void *p;
        size_t bytes;
    };
    static int track_measure_spans(const TrackJob &j, ZeroSpan spans[3]);
    int admit_job(TrackJob &j, TrackBufs &acc, const TrackOptions &opt, const float *audio, int rate, int length_at_rate, bool leaves_whole);
    void track_leave(TrackJob &j, float *const src[4], size_t src_start, int count, long long first_frame, hipStream_t st);
    struct TrackReport // what a job measured, on the host (track_report); only what its options asked for is filled
    {
        umx_levels lv = {};
        umx_loudness ld = {};
        std::vector<double> hopE;
        umx_true_peak tp = {};
    };
    hipError_t track_report(const TrackJob &j, int n_host, TrackReport &r);
    hipError_t track_upload_until(TrackJob &j, long long padded_end, hipStream_t st);
    void track_mix(const MixSpec &mix, float *const stems[4], size_t stem_start, const float *in, size_t in_start, int count, hipStream_t st);
    hipError_t track_region_download(const TrackRegion &r, float *const *out_host);
    int track_call(const TrackLane *lanes, int nl, unsigned flags, int &last_slot, TrackRegions &regions);
    // track queue (engine_queue.h): B + 2 accumulator sets (in, out, sumw of TrackBufs; grow-only) lent to the jobs in flight
    std::vector<TrackBufs> qpool;
    int queue_calls = -1; // infer_batch calls of the last queue run
    struct QueueDone // the done callback of a run: the plain one, or the one that receives every job's levels, or (DESIGN
    {               // 21) the one that also receives the loudness record and the hop energies, or the true-peak record as well
        umx_queue_done_fn plain = nullptr;
        umx_queue_levels_fn with_levels = nullptr;
        umx_queue_loudness_fn with_loudness = nullptr;
        umx_queue_true_peak_fn with_true_peak = nullptr;
        explicit operator bool() const { return plain || with_levels || with_loudness || with_true_peak; }
        // what the callback implies for every job of the run (opt.levels, opt.loudness): a wider callback receives the narrower records too
        bool measures() const { return with_levels || loudness(); }
        bool loudness() const { return with_loudness || with_true_peak; }
        void call(void *user, const umx_queue_job *job, const TrackReport &r) const
        {
            if (with_true_peak)
                with_true_peak(user, job, &r.lv, &r.ld, r.hopE.data(), &r.tp);
            else if (with_loudness)
                with_loudness(user, job, &r.lv, &r.ld, r.hopE.data());
            else if (with_levels)
                with_levels(user, job, &r.lv);
            else
                plain(user, job);
        }
    };
    int queue(umx_queue_next_fn next, const QueueDone &done, void *user, const TrackOptions &opt, unsigned flags);
    int queue_run(umx_queue_next_fn next, const QueueDone &done, void *user, const TrackOptions &opt, unsigned flags);
    int phase_begin(const float *audio_host, int n, unsigned flags);
    int phase_begin_device(const float *audio_dev, int n, unsigned flags);
    int phase_end_device(float *const out_dev_[4]);
    const float *ph_audio = nullptr;
    int phase_layer(int layer);
    int phase_end(float *const out_host[4]);
    int ph_next = -1; // -1: no phased segment open; 0..2: next LSTM layer; 3: back stage pending
    int ph_n = 0;
    unsigned ph_flags = 0;
    template <class Args> void fill_lstm_args(Args &a, Slot &sl, int layer, const int *active, int nact);
    int run_lstm_layer(Slot &sl, int layer, const int *active, int nact, bool stepwise, unsigned long long lane_mask);
    int run_lstm_layer_batched(Slot &sl, int layer, const int *active, int nact, bool stepwise, unsigned long long lane_mask);
    int sync_all();
    void launch_gemm(Lane &ln, hipStream_t st, int mode, int layer, const int *active, int nact, bool dbg);
    int stage_front(Slot &sl, hipStream_t st, int nb, const float *const *audio_dev, const int *n, const int *active, int nact);
    // elements between the streaming buffers of consecutive track lanes of a slot (the kernels take lane 0's pointers)
    WienerStrides lane_strides() const
    {
        WienerStrides ls;
        const size_t nchunk = (size_t)(T + WIENER_CHUNK - 1) / WIENER_CHUNK;
        ls.spec = (size_t)2 * T * NBINS;
        ls.mag = (size_t)2 * T * MAGP;
        ls.part = std::max((size_t)4 * nbatch * NBINS * 9, nchunk * 4 * 5 * NBINS);
        ls.rc = (size_t)4 * NBINS * 4;
        ls.frames = (size_t)4 * T * NFFT;
        ls.y = (size_t)4 * 2 * T * NBINS;
        ls.v = (size_t)4 * T * NBINS;
        return ls;
    }
    static LaneSet lane_set(int nb, const float *const *audio_dev) // the active lanes of a call
    {
        LaneSet l;
        l.count = 0;
        for (int ln = 0; ln < nb; ++ln)
            if (audio_dev[ln])
                l.id[l.count++] = (unsigned char)ln;
        return l;
    }
    int stage_back(Slot &sl, hipStream_t st, int nb, const float *const *audio_dev, float *const *out, const int *n,
                   unsigned flags, const int *active, int nact);
    // its two halves: fc2 + fc3 -> the target magnitudes of the active targets | Wiener (or mixture phase), inverse STFT,
    // overlap-add from the magnitudes of ALL four targets (zero_skipped: a skipped target counts as silence; false when
    // its magnitudes were put there by someone else -- the target-sharded multi-GPU driver)
    int stage_masks(Slot &sl, hipStream_t st, int nb, const float *const *audio_dev, unsigned flags, const int *active, int nact);
    int stage_finish(Slot &sl, hipStream_t st, int nb, const float *const *audio_dev, float *const *out, const int *n, unsigned flags,
                     bool zero_skipped);
    int phase_masks();
    int phase_residual();
    int phase_finish_device(float *const out_dev_[4]);
    // UMX_FLAG_RESIDUAL: the one check of the flag combination every entry point that takes flags goes through.
    // UMX_FLAG_SOFTMASK goes with every combination that passes: it normalises whatever targets are active (none: nothing to do).
    int check_flags(unsigned flags)
    {
        if (residual_slot_of(flags) != -2)
            return UMX_OK;
        set_error("UMX_FLAG_RESIDUAL needs at least one skipped target (UMX_FLAG_SKIP_TARGET: its slot carries the residual; four targets "
                  "plus a residual would be five sources) and at least one active target");
        return UMX_ERR_ARG;
    }
    // UMX_FLAG_SOFTMASK: the active targets' masks normalised in place, all lanes of the call in one launch (softmask.h)
    void stage_softmask(Slot &sl, hipStream_t st, int nb, const float *const *audio_dev, const int *active, int nact);
    // rho of the residual slot from the active targets' masks, all lanes of the call in one launch (residual_mask.h)
    int stage_residual(Slot &sl, hipStream_t st, int nb, const float *const *audio_dev, unsigned flags);
    static void active_list(unsigned flags, int *active, int &nact)
    {
        nact = 0;
        for (int tg = 0; tg < 4; ++tg)
            if (!(flags & UMX_FLAG_SKIP_TARGET(tg)))
                active[nact++] = tg;
    }
    // shift ensemble (shift_mean.h): TrackRequest::ensemble = the lanes are ONE track (audio[0], length[0], rate[0])
    // at n_tracks shift offsets, `out` its 4 stems: one upload, the lanes' stems averaged on the device into ens_out (grow-only), one
    // download.  Only umx_hip_shift_ensemble with more than one shift touches these.
    float *ens_out[4] = {};
    size_t ens_cap = 0;          // frames
    hipEvent_t ens_ev[2] = {};   // around shift_mean_kernel of the last ensemble (umx_hip_debug_shift_mean_ms)
    bool ens_timed = false;
};

#include "engine_init.h"
#include "engine_lstm.h"
#include "engine_stages.h"
#include "engine_tracks.h"
#include "engine_queue.h"
#include "engine_phased.h"
#include "engine_cabi.h"
