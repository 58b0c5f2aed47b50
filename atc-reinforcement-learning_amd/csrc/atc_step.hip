// atc_step.hip — libatcstep.so: hand-written gfx950 (CDNA4, MI355X) kernels + C-ABI of the batched AtcGym.step() path.
//
// Work decomposition: lane = one aircraft slot, W = next_pow2(N) consecutive lanes = one env, 64 / W envs per wavefront; workgroup =
// 256 consecutive slots, one per tile, no block barrier, no atomics in the fast variant, no MFMA (no contraction on this path).
//   State in HBM (include/atc_step.h, ABI 20): ac = (x, y on the 32-bit position grid, heading counts, speed counts) 16 B, alt = the
//   altitude as the reference's float64 8 B, last_act 16 B (touched only by steps that may change it), a 16-byte env record shared
//   by the W lanes of an env; every array moves with ONE access per lane on consecutive addresses, 32-bit offsets from uniform bases.
//   The sector blob stays in global memory: constants through scalar loads, the MVA lookup one 8-byte gather per aircraft (+ edge
//   records in cells a border cuts).  No staging prologue: the first thing a wavefront does is issue its state loads.
//   Separation scan, every unordered pair once: N = 16 one DPP row per env (row rotation fused into the subtract, the inverse
//   rotation hands the result back); N <= 8 XOR partners through quad_perm / row_half_mirror; N > 16 LDS planes + packed fp32 +
//   ballot masks rotated on the scalar unit.  Per-env sums by DPP butterflies, done / won masks by ballot.
//   The single-step kernel has NO loop around the step body (its own instantiation, ONE); multi-step launches keep the state in
//   registers across a run-time step loop under an 80-VGPR bound; LAT is their form for at most two wavefronts per SIMD; k_serve
//   is the resident one-env step server.  How each choice was measured: DESIGN_HISTORY.md, profiles/experiments/.
//
// Build: hipcc --offload-arch=gfx950 -O3 -ffp-contract=off -fPIC -shared   (see build.py)
#include <hip/hip_runtime.h>
#include <atomic>
#include <chrono>
#include <sched.h>
#include <stdarg.h>
#include <emmintrin.h>   // host side of atc_step_packet: 16-byte loads of the mapped result packet
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <type_traits>

#include "atc_device.h"
#include "atc_kernarg.h"

using namespace atc;

struct atc_scenario {
    float* d_blob;   // device copy of the whole blob (constants + polygons + entries [+ grid])
    int n_words;
    int off_grid;    // 0 = no grid
    int device;
    int n_cu;
    float consts[ATC_C_END];   // host copy of the blob's header + constants block (derive() evaluates uniform terms from it)
    float ghdr[ATC_G_HDR];     // host copy of the lookup grid's header (zeros without a grid)
    uint64_t uid;              // unique per created handle (never reused: keys the per-thread cache of derive())
    void* d_lds;               // LDS-resident lookup table (atc_scenario_attach_lds_table): device copy, or null
    LdsTab lt;                 // ... and the kernel argument that describes it (src == null: none)
    size_t lds_tab_bytes;
    int max_lds;               // the device's LDS bytes per workgroup
    int cu_lds;                // ... and per CU (what the workgroups resident on a CU share)
};

static thread_local char g_err[512] = "";

#define ATC_OK 0
#define ATC_ERR_ARG (-1)
#define ATC_ERR_HIP (-2)

static int fail_arg(const char* msg) {
    snprintf(g_err, sizeof g_err, "bad argument: %s", msg);
    return ATC_ERR_ARG;
}
// a refusal with the call's own words in it: formatted here, so only ever on the refusing path
__attribute__((format(printf, 1, 2))) static int fail_argf(const char* fmt, ...) {
    char msg[160];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(msg, sizeof msg, fmt, ap);
    va_end(ap);
    return fail_arg(msg);
}
static int fail_hip(hipError_t e, const char* what) {
    snprintf(g_err, sizeof g_err, "HIP error in %s: %s", what, hipGetErrorString(e));
    (void)hipGetLastError();  // reported here: do not leave it as the runtime's sticky "last error" for the caller's framework
    return ATC_ERR_HIP;
}
#define HIP_TRY(expr)                                    \
    do {                                                 \
        hipError_t _e = (expr);                          \
        if (_e != hipSuccess) return fail_hip(_e, #expr); \
    } while (0)

// Rejected / default-off variants of rounds 1-5 (scan forms, ablation masks, store orders, ...) were moved out of this file in
// round 6: profiles/experiments/ holds the patch that restores them and one line per measurement.
// Wave-uniform conditions that almost never hold (or almost always): the hint moves the rare block out of the step's straight
// line, so that the common path FALLS THROUGH its branches instead of jumping over code (a taken branch refills the
// instruction buffer: ~20 cycles to a wavefront alone on its SIMD, tools/ubench/valu_rates.hip).
#define ATC_RARE(x) __builtin_expect(!!(x), 0)
#define ATC_USUAL(x) __builtin_expect(!!(x), 1)
constexpr int kBlock = 256;
#ifndef ATC_TRACE
#define ATC_TRACE 0  // developer-only: per-wavefront s_memtime stamps at phase boundaries (pointer smuggled in params)
#endif
#if ATC_TRACE
// one row of 8 stamps per wavefront AND step (row = wavefront * steps + step)
#ifndef ATC_TRACE_MODE
#define ATC_TRACE_MODE 0   // 0: the step's phases (tools/trace_rollout.py); 1: stamps 1..5 dissect the step's first phase instead
#endif                     // 3: mode 0 with stamp 1 taken when the state has ARRIVED (behind the rate limits): tools/trace_fill.py
#define ATC_STAMP_AT(row, n) do { if ((threadIdx.x & 63) == 0 && (row)) (row)[(n)] = __builtin_amdgcn_s_memtime(); } while (0)
#define ATC_STAMP(n) do { if (ATC_TRACE_MODE == 0 || (ATC_TRACE_MODE == 3 && (n) != 1)) ATC_STAMP_AT(trow, n); } while (0)
#define ATC_STAMP_B(n) do { if (ATC_TRACE_MODE == 0 || ATC_TRACE_MODE == 3) ATC_STAMP_AT(so.trace, n); } while (0)
#define ATC_STAMP_TOP(row, n) do { if (ATC_TRACE_MODE == 1) ATC_STAMP_AT(row, n); else if (ATC_TRACE_MODE == 3 && (n) == 2) ATC_STAMP_AT(row, 1); } while (0)
#define ATC_STAMP_END(row, n) do { if (ATC_TRACE_MODE == 2) ATC_STAMP_AT(row, n); } while (0)   // mode 2: the step's LAST phase dissected
#define ATC_TRACE_PARAM , unsigned long long* trace_row
#define ATC_TRACE_PASS(x) , (x)
#else
#define ATC_STAMP(n) do {} while (0)
#define ATC_STAMP_B(n) do {} while (0)
#define ATC_STAMP_TOP(row, n) do {} while (0)
#define ATC_STAMP_END(row, n) do {} while (0)
#define ATC_TRACE_PARAM
#define ATC_TRACE_PASS(x)
#endif
// Multi-step launches of the DPP widths re-read the STATE pointers from the kernarg segment after the step loop (see StepArgs)
// instead of carrying them across it; the LDS-scan widths name them (measured per width: profiles/r02_experiments.txt).
constexpr bool loop_rereads_state(int W) { return W < 32; }
#define ATC_GRID_CAP 8        // workgroups per CU before the reset / observe / query kernels grid-stride
#define ATC_MIN_WAVES 4       // waves per SIMD the single-step kernel is register-budgeted for (<= 128 VGPRs; it needs 55-72)
#define ATC_MIN_WAVES_LOOP 6  // multi-step launches: <= 80 VGPRs.  Without the bound the allocator keeps literal constants and
                              // other loop invariants in registers across the step loop (86-99 VGPRs, 4-5 waves per SIMD)

#include "atc_wave.h"   // group reductions (DPP butterflies) and the DPP separation scans

// Per-lane addressing = uniform 64-bit base + 32-bit BYTE offset (the host guarantees B*N*40 < 4 GiB): the compiler can
// then use the scalar-base addressing form and does not keep a 64-bit address pair per array alive in VGPRs.
template <typename T>
__device__ __forceinline__ T* at(void* base, uint32_t byte_off) {
    return reinterpret_cast<T*>(reinterpret_cast<char*>(base) + byte_off);
}
template <typename T>
__device__ __forceinline__ const T* at(const void* base, uint32_t byte_off) {
    return reinterpret_cast<const T*>(reinterpret_cast<const char*>(base) + byte_off);
}
// Byte offsets of 12- and 40-byte records as shift-adds: the compiler multiplies (v_mul_lo_u32 is a quarter-rate instruction,
// and lane indices do not fit the 24-bit multiplier); asm keeps the two full-rate instructions from being folded back.
__device__ __forceinline__ uint32_t times12(uint32_t i) {
    uint32_t t;
    asm("v_lshl_add_u32 %0, %1, 1, %1" : "=v"(t) : "v"(i));   // 3 i
    return t << 2;
}
__device__ __forceinline__ uint32_t times40(uint32_t i) {
    uint32_t t;
    asm("v_lshl_add_u32 %0, %1, 2, %1" : "=v"(t) : "v"(i));   // 5 i
    return t << 3;
}
// write-once output streams (observation, flag words) are stored non-temporal: 30.7 vs 31.9 us at 65 536 x 16 (r01)
template <typename T>
__device__ __forceinline__ void stream_store(T* p, T v) {
    __builtin_nontemporal_store(v, p);
}
// One 16-byte store written THROUGH to system memory (sc0 sc1): a chunk of the result packet a host polls in mapped memory.  A plain
// store to host memory may stay in the device's L2 until the kernel ends — which a resident kernel (k_serve) never does.
__device__ __forceinline__ void store16_system(uint4* p, uint32_t a, uint32_t b, uint32_t c, uint32_t d) {
    typedef uint32_t v4u __attribute__((ext_vector_type(4)));
    const v4u v = {a, b, c, d};
    asm volatile("global_store_dwordx4 %0, %1, off sc0 sc1" : : "v"(p), "v"(v) : "memory");
}
__device__ __forceinline__ void store_obs(float* __restrict__ dst, const float* o) {
    // 10 floats = 40 B per aircraft: 8-byte aligned -> five 8-byte stores
    float2* d = reinterpret_cast<float2*>(dst);
#pragma unroll
    for (int c = 0; c < 5; ++c) d[c] = make_float2(o[2 * c], o[2 * c + 1]);
}

// ---------------------------------------------------------------------------------------------------------------
// step / rollout kernel
//   FULL = false : the fast variant — obs, reward, done, flags only (what step() returns); the optional outputs
//                  (raw_obs, ac_reward, min_sep, term_obs) and their pointers are compiled out.
//   One workgroup handles 256 consecutive slots (no grid-stride loop: with a loop the compiler hoists the uniform loads
//   out of it and spills the scalar registers that then stay live across the whole body).
//   The body is straight-line for every lane: lanes whose aircraft is not under control compute on their frozen state and
//   the results are discarded by selects; only the rare paths (dirty grid cells, corridor interior, auto-reset) branch.
// ---------------------------------------------------------------------------------------------------------------
struct LaneIds {        // who this lane is (one aircraft slot of one env)
    int tid, lane, e, k;
    uint32_t i;         // aircraft index env * N + k (clamped into range for lanes without an aircraft)
    uint32_t slot0;     // first slot of the workgroup's tile
    bool env_valid, lane_valid, wave_full;
};
struct LaneState {      // persistent per-aircraft state held in registers
    Aircraft a;
    uint32_t la_v;      // last accepted targets (atc_gym.py:86,311) in the state's formats: speed counts,
    double la_h;        // altitude [ft] (float64),
    int la_p;           // heading counts
    bool la_changed;
};
struct Targets {        // decoded action of the current step / block (atc_gym.py:318-335) in the state's formats
    uint32_t v;
    float ah;           // the altitude's ACTION: its float64 target a * m + c is evaluated where it is used (one conversion and
    int p;              // one fma per step instead of a register pair carried across a held block)
};
struct EnvState {       // per-step env record (replicated in the W lanes of the env)
    int t, n_actions;
    float total_reward;
    uint64_t amask;     // bits 32..63 live in the per-episode record and exist only for envs of more than 32 aircraft
};
struct Float3 {
    float a, b, c;
};
struct Mid {            // what the first half of a step hands to the second
    bool active;
    float r;
    uint32_t fl;
    int acts;
    float x32, y32;
    MvaCell cell;       // MVA lookup cell, gather issued in the first half, resolved after the separation scan
    LdsCode lc;         // ... or its codes in the LDS-resident table (LDSG instantiation)
    bool repeated;      // uniform: no action bookkeeping in this step (acts == 0 in every lane)
    bool plain;         // uniform: every lane flies an aircraft under control towards valid targets (fl == 0, no refusal)
};
// Uniform products of the step parameters, evaluated ONCE on the host in fp32 (the same IEEE operations the kernel
// would do) and passed as kernel arguments: gfx950 has no scalar float ALU, so computed in the kernel they would occupy
// vector registers — and a multi-step launch would keep them there across its whole step loop.
// Grouped by the stage that consumes them: a multi-step launch re-reads each group from the kernarg segment right where its
// stage starts (QGET below) instead of keeping ~70 uniform values alive across the step loop.
struct alignas(16) QRates {   // first half of the step (20 words)
    // _denormalized_action (atc_gym.py:318-335) for the fixed-point components: counts = trunc(a * m + c) in float64 (m, c the
    // reference's factor / offset in counts: integers), see decode_targets
    double dec_mv, dec_cv, dec_mp, dec_cp;
    double dec_mh, dec_ch;  // altitude target (float64): a * m + c as one fma = the reference's operation order (see derive())
    double dh_hi, dh_lo;    // kHDotMax * dt, kHDotMin * dt in float64 (model.py:45-46,97-100)
    int rate_v, rate_p;     // rint(kAMax dt 2^23), rint(kPhiDotMax dt 2^23): symmetric limits (model.py:47-50,75-78,113-120)
    float r_base;           // -0.05 * dt                       (atc_gym.py:137)
    int pos_neg_k;          // position grid: nm = origin + fix * 2^-k (blob: ATC_C_POS_*)
};
struct alignas(16) QGrid {    // position conversion + MVA cell lookup
    double pos_x0, pos_y0;
    GridHdr gh;           // lookup grid header (7 words)
    int pad;
};
struct alignas(16) QScan {    // second half: separation scan, override chain
    float sep2;           // sep_nm ^ 2
    float sep_ft, conflict_reward;
    int timestep_limit;
    float4 tri_bbox;      // bounds of the corridor's horizontal triangle (ATC_C_TRI_BBOX)
    int n_noise;          // number of noise-abatement areas (blob header word; read from the blob inside the step it was a
    int off_spawn;        // dependent scalar load with nothing to hide its latency behind, in every step of every wavefront);
                          // word offset of the blob's spawn records (ATC_H_OFF_SPAWN)
    float sep2_h, sep_ft_h;   // the minima with the closing distance of the launch's scan horizon added (scan_horizon_limits)
};
struct alignas(16) QNorm {
    float a[ATC_OBS_DIM], b[ATC_OBS_DIM];   // ATC_C_NORM_A / ATC_C_NORM_B
};
struct alignas(64) StepDerived {
    QRates r;
    QKin k;               // float64 heading kinematics + distance scale (32 words)
    QGrid g;
    QScan s;
    ObsConst oc;          // observation / shaping constants
    int pad[2];
    QNorm n;
};
// LAT — the latency-bound instantiation of the multi-step kernels, for launches of at most two wavefronts per SIMD (65 536 x 1,
// 8 192 x 16: every BASELINE configuration but the headline and 4 096 x 64).  There a step IS one wavefront's serial instruction
// chain and the vector register file is all but empty, so the uniform FLOATING-POINT terms of StepDerived (~80 words) are copied
// into vector registers once per launch — every lane holds the same value — and the step loop reads them as ordinary operands:
// no kernarg re-read (a scalar load and its wait: ~45 cycles for a wavefront alone, 17 per step at W = 1), no scalar register
// spilled to lanes, no constant-bus limit.  Integer terms that steer scalar control flow stay scalar.
__device__ __forceinline__ float vg(float x) {
    float r;
    asm("v_mov_b32 %0, %1" : "=v"(r) : "s"(x));
    return r;
}
__device__ __forceinline__ double vg(double x) {
    int lo, hi;
    asm("v_mov_b32 %0, %1" : "=v"(lo) : "s"(__double2loint(x)));
    asm("v_mov_b32 %0, %1" : "=v"(hi) : "s"(__double2hiint(x)));
    return __hiloint2double(hi, lo);
}
__device__ __forceinline__ int vg(int x) {
    int r;
    asm("v_mov_b32 %0, %1" : "=v"(r) : "s"(x));
    return r;
}
__device__ __forceinline__ StepDerived to_vector_registers(const StepDerived& q) {
    StepDerived v = q;
    // (integers that are only ever VALU operands — limits, grid dimensions, the FAF's grid coordinates — go along: each frees a scalar
    // register the loop would otherwise spill to a vector-register lane and read back with v_readlane)
    v.r.rate_v = vg(q.r.rate_v); v.r.rate_p = vg(q.r.rate_p); v.r.pos_neg_k = vg(q.r.pos_neg_k);
    v.g.gh.nx = vg(q.g.gh.nx); v.g.gh.nx_last = vg(q.g.gh.nx_last); v.g.gh.ny_last = vg(q.g.gh.ny_last);
    v.oc.faf_x = vg(q.oc.faf_x); v.oc.faf_y = vg(q.oc.faf_y);
    v.s.timestep_limit = vg(q.s.timestep_limit);
    v.r.dec_mv = vg(q.r.dec_mv); v.r.dec_cv = vg(q.r.dec_cv); v.r.dec_mp = vg(q.r.dec_mp); v.r.dec_cp = vg(q.r.dec_cp);
    v.r.dec_mh = vg(q.r.dec_mh); v.r.dec_ch = vg(q.r.dec_ch);
    v.r.dh_hi = vg(q.r.dh_hi); v.r.dh_lo = vg(q.r.dh_lo); v.r.r_base = vg(q.r.r_base);
    v.k.inv180 = vg(q.k.inv180); v.k.neg_half_turn = vg(q.k.neg_half_turn);
    v.k.s0 = vg(q.k.s0); v.k.s1 = vg(q.k.s1); v.k.s2 = vg(q.k.s2); v.k.s3 = vg(q.k.s3); v.k.s4 = vg(q.k.s4); v.k.s5 = vg(q.k.s5);
    v.k.c1 = vg(q.k.c1); v.k.c2 = vg(q.k.c2); v.k.c3 = vg(q.k.c3); v.k.c4 = vg(q.k.c4); v.k.c5 = vg(q.k.c5);
    v.k.dist_neg = vg(q.k.dist_neg);
    v.g.pos_x0 = vg(q.g.pos_x0); v.g.pos_y0 = vg(q.g.pos_y0);
    v.g.gh.x0 = vg(q.g.gh.x0); v.g.gh.y0 = vg(q.g.gh.y0); v.g.gh.inv = vg(q.g.gh.inv);
    v.s.sep2 = vg(q.s.sep2); v.s.sep_ft = vg(q.s.sep_ft); v.s.conflict_reward = vg(q.s.conflict_reward);
    v.s.sep2_h = vg(q.s.sep2_h); v.s.sep_ft_h = vg(q.s.sep_ft_h);
    v.oc.pos_inv = vg(q.oc.pos_inv); v.oc.to_rwy = vg(q.oc.to_rwy); v.oc.on_gp_c = vg(q.oc.on_gp_c); v.oc.sig_a = vg(q.oc.sig_a);
#pragma unroll
    for (int c = 0; c < ATC_OBS_DIM; ++c) { v.n.a[c] = vg(q.n.a[c]); v.n.b[c] = vg(q.n.b[c]); }
    return v;
}

// atc_step_packet: the ONE env's action by value, a kernel argument of its own (no read over the host link on the device side)
struct InlineAction {
    float v, h, p;
    int set;
};
static thread_local const float* t_inline_action = nullptr;   // set by atc_step_packet around its launch
static InlineAction inline_action() {
    InlineAction a = {0.0f, 0.0f, 0.0f, 0};
    if (t_inline_action) a = InlineAction{t_inline_action[0], t_inline_action[1], t_inline_action[2], 1};
    return a;
}
static StepDerived derive_uncached(const atc_params_t& p, const atc_scenario* s, int horizon);
// The uniform terms depend on the sector and on a few parameters only; a caller steps the same env thousands of times with the
// same ones, so each thread remembers its last evaluation (the single-env path launches one tiny kernel per step: the
// evaluation would be a measurable part of its host time).  Thread-local: the library stays free of shared mutable state.
// `horizon`: the steps a multi-step launch may leave the separation scan out after one that found every pair far apart (0: none)
static const StepDerived& derive(const atc_params_t& p, const atc_scenario* s, int horizon) {
    struct Key {
        uint64_t uid;
        double dt;
        float sep_nm, sep_ft, conflict_reward;
        int32_t timestep_limit;
        uint32_t mode_bits;   // the mode flags the derived values depend on
        int32_t horizon;
    };
    static thread_local Key last = {0ull, 0.0, 0.0f, 0.0f, 0.0f, 0, 0u, 0};
    static thread_local StepDerived q;
    const Key k = {s->uid, p.dt, p.sep_nm, p.sep_ft, p.conflict_reward, p.timestep_limit, p.mode & (uint32_t)(ATC_M_DISCRETE | ATC_M_NORMALIZE), horizon};
    if (memcmp(&k, &last, sizeof k) != 0) {
        q = derive_uncached(p, s, horizon);
        last = k;
    }
    return q;
}
// Separation scan horizon (include/atc_step.h): thresholds S2 >= sep_nm^2 and SF >= sep_ft such that a pair of aircraft with
//   d^2 >= S2  or  |dh| >= SF     (d^2, dh as the scan evaluates them, fp32)
// now cannot satisfy (d^2 < sep_nm^2 and |dh| < sep_ft) in any of the next n steps.  Per step an aircraft moves by at most
// (v / 3600) dt (1 + 1e-9) nm + one position count per axis (advance(): |sin|, |cos| <= 1 + 1e-9, floor of displacement + dither) with
// v <= 300 kt as long as it is at most 300 kt now (valid targets lie in [100, 300], the rate-limited move never overshoots: the scan
// checks the speeds it starts from), and its altitude by at most 15 dt up / 41 dt down + half an ulp (the scan checks |h| < 2^17 ft:
// ulp <= 2^-6 ft).  So d shrinks by at most 2 (300 / 3600) dt and |dh| by at most 56 dt per step; the slack terms — 1e-5 relative
// + 1e-3 nm, 1e-5 relative + 1 ft — are hundreds of times the fp32 evaluation error of d^2 (a few ulp + 2^-17 nm per coordinate).
// Aircraft that are handed over stay where they are until their env is reset, and a reset ends the horizon (step_part_b).
static void scan_horizon_limits(const atc_params_t& p, int n, float* sep2_h, float* sep_ft_h) {
    const float sep2 = p.sep_nm * p.sep_nm;
    *sep2_h = sep2;
    *sep_ft_h = p.sep_ft;
    if (n <= 0) return;
    const double dt = p.dt;
    const double S = (sqrt((double)sep2) + n * 2.0 * ((double)kVMax / 3600.0) * dt) * (1.0 + 1e-5) + 1e-3;
    const double F = ((double)p.sep_ft + n * ((double)kHDotMax - (double)kHDotMin) * dt) * (1.0 + 1e-5) + 1.0;
    float s2 = (float)(S * S), f = (float)F;
    if ((double)s2 < S * S) s2 = nextafterf(s2, INFINITY);
    if ((double)f < F) f = nextafterf(f, INFINITY);
    // (NaN parameters: every compare of the scan is false either way; thresholds that did not come out above the minima — overflow,
    // NaN — become +inf: "some pair is near" in every scan, i.e. no step is skipped)
    *sep2_h = (s2 >= sep2) ? s2 : INFINITY;
    *sep_ft_h = (f >= p.sep_ft) ? f : INFINITY;
}
static StepDerived derive_uncached(const atc_params_t& p, const atc_scenario* s, int horizon) {
    const float* K = s->consts;
    StepDerived q;
    memset(&q, 0, sizeof q);
    int k_pos;
    {
        int e = 0;
        (void)frexpf(K[ATC_C_POS_SCALE], &e);   // 2^k = 0.5 * 2^(k + 1)
        k_pos = e - 1;
        q.r.pos_neg_k = -k_pos;
    }
    q.g.pos_x0 = (double)K[ATC_C_POS_X0];
    q.g.pos_y0 = (double)K[ATC_C_POS_Y0];
    const double dtd = p.dt, fixq = 8388608.0;   // 2^23: speed and heading counts per kt / deg
    auto rate_fix = [&](float rate) {   // rint(|rate| dt 2^23), saturating (include/atc_step.h)
        const double r = rint(fabs((double)rate) * dtd * fixq);
        return r >= 2147483647.0 ? INT32_MAX : (int32_t)r;
    };
    q.r.rate_v = rate_fix(kAMax);
    q.r.rate_p = rate_fix(kPhiDotMax);
    q.r.dh_hi = (double)kHDotMax * dtd;   // h_dot_max * timestep: an integer times a Python float (model.py:97-100)
    q.r.dh_lo = (double)kHDotMin * dtd;
    q.r.r_base = (float)(-0.05 * dtd);
    // atc_gym.py:64-78,318-335: offset (v_min, 0, 0); factor (10, 100, 1) discrete | (v_max - v_min, h_max, 360) continuous.
    //   discrete   : a * fac + off
    //   continuous : a * fac / 2 + fac / 2 + off
    // Speed and heading (fixed point): counts = a * m + c evaluated as ONE float64 fma — exact for every fp32 action in the
    // action space (24 x 31 bits) — and truncated; m = the factor, c = the offset relative to the format's origin, in counts.
    const bool discrete = (p.mode & ATC_M_DISCRETE) != 0;
    q.r.dec_mv = (discrete ? 10.0 : (double)(kVMax - kVMin) / 2.0) * fixq;
    q.r.dec_cv = (discrete ? (double)kVMin : (double)(kVMax - kVMin) / 2.0 + (double)kVMin) * fixq;
    q.r.dec_mp = (discrete ? 1.0 : 360.0 / 2.0) * fixq;
    q.r.dec_cp = ((discrete ? 0.0 : 360.0 / 2.0) - (double)ATC_PHI_FIX_OFFSET) * fixq;
    // Altitude (float64, ABI 20): the product of an fp32 action with fac (38 000: 16 bits) is exact in float64 and halving is
    // exact, so a * fac / 2 + fac / 2 + 0 is ONE rounding — the fma's (the discrete form keeps its `+ 0`: it turns a -0 product
    // into +0, like the reference's `+ offset`).
    q.r.dec_mh = discrete ? 100.0 : (double)kHMax / 2.0;
    q.r.dec_ch = discrete ? 0.0 : (double)kHMax / 2.0;
    // float64 heading kinematics (include/atc_step.h: ATC_KIN_*) and the step's distance scale, NEGATED (see atc::advance)
    q.k.inv180 = ATC_KIN_INV180;
    q.k.neg_half_turn = -ATC_KIN_HALF_TURN;
    q.k.s0 = ATC_KIN_S0; q.k.s1 = ATC_KIN_S1; q.k.s2 = ATC_KIN_S2; q.k.s3 = ATC_KIN_S3; q.k.s4 = ATC_KIN_S4; q.k.s5 = ATC_KIN_S5;
    q.k.c1 = ATC_KIN_C1; q.k.c2 = ATC_KIN_C2; q.k.c3 = ATC_KIN_C3; q.k.c4 = ATC_KIN_C4; q.k.c5 = ATC_KIN_C5;
    q.k.dist_neg = -ldexp(dtd / 3600.0, k_pos - ATC_V_FIX_SHIFT);
    q.g.gh = grid_header(s->off_grid ? s->ghdr : nullptr);
    q.s.sep2 = p.sep_nm * p.sep_nm;
    q.s.sep_ft = p.sep_ft;
    scan_horizon_limits(p, horizon, &q.s.sep2_h, &q.s.sep_ft_h);
    q.s.conflict_reward = p.conflict_reward;
    q.s.timestep_limit = p.timestep_limit;
    q.s.tri_bbox = make_float4(K[ATC_C_TRI_BBOX], K[ATC_C_TRI_BBOX + 1], K[ATC_C_TRI_BBOX + 2], K[ATC_C_TRI_BBOX + 3]);
    q.s.n_noise = (int)K[ATC_H_N_NOISE];
    q.s.off_spawn = (int)K[ATC_H_OFF_SPAWN];
    q.oc = obs_const(K);
    // atc_gym.py:187-189.  Without ATC_M_NORMALIZE the same fma runs with (1, -0): x * 1 + -0 == x for every x, signed
    // zeros included — the step has no branch on the flag and the constants can be requested ahead of the observation.
    const bool normalize = (p.mode & ATC_M_NORMALIZE) != 0;
    for (int c = 0; c < ATC_OBS_DIM; ++c) {
        q.n.a[c] = normalize ? K[ATC_C_NORM_A + c] : 1.0f;
        q.n.b[c] = normalize ? K[ATC_C_NORM_B + c] : -0.0f;
    }
    return q;
}

// k_step's argument list as a struct: the kernarg segment is laid out by the same rules, so offsetof() names where an
// argument lives.  Multi-step launches RE-READ their by-value arguments (output pointers, parameters, derived constants, the state
// pointers needed again after the loop) from the kernarg segment inside the step instead of keeping ~60 SGPRs of them alive
// across the loop: the allocator spills those to VGPR lanes and every use becomes a v_readlane — VALU work in a launch that is
// bound by VALU issue — whereas a kernarg re-read is a scalar load.  The offset goes through an opaque zero, or the (invariant)
// loads would be hoisted out of the loop again.
//   The step halves are shared by every multi-step kernel, so each of those kernels must put what they re-read where StepArgs says.
//   The only description of a kernel's layout is its parameter list (KernArgs, atc_kernarg.h): StepArgs is held to k_step's list behind
//   k_step, and every other kernel's list to StepArgs by kernargs_like_step in a static_assert directly behind the kernel.
struct StepArgs {
    const float* blob;
    int off_grid, B, N, T, hold;
    atc_state_t st;
    const float* actions;
    atc_out_t out;
    atc_params_t p;
    StepDerived q;
    InlineAction ia;
    LdsTab lt;
    int pf_stride;   // fill-phase prefetch (k_step): behind everything k_skip's argument list shares with this one
};
// F's first atc_state_t, its atc_out_t and its StepDerived lie where k_step's do
template <typename F>
constexpr bool kernargs_like_step() {
    typedef KernArgs<F> A;
    return A::template of<atc_state_t>() == offsetof(StepArgs, st) && A::template of<atc_out_t>() == offsetof(StepArgs, out) &&
           A::template of<StepDerived>() == offsetof(StepArgs, q);
}
// ... and F's parameter 5 is `hold`: it lies where k_step's does, directly in front of the state (parameters have no names in a type: an
// int put anywhere in front of `st` moves the state off index 6, or off its offset)
template <typename F>
constexpr bool kernargs_hold_like_step() {
    typedef KernArgs<F> A;
    return kernargs_like_step<F>() && A::template at<5>() == offsetof(StepArgs, hold) && A::template at<6>() == A::template of<atc_state_t>();
}
#define ATC_KERNARGS_REFUSAL "the kernel's arguments must lie where k_step's do: the step re-reads them by StepArgs offsets"
template <typename T>
__device__ __forceinline__ T kernarg_reread(size_t byte_off, int opaque_zero) {
#if __HIP_DEVICE_COMPILE__   // (the host pass only parses this body; the builtin exists for the device target)
    // A TYPED load through the constant address space: the alignment of T is then known to the compiler, which it needs
    // for scalar loads (a byte-wise copy from an address with an opaque term became per-lane vector loads).
    typedef __attribute__((address_space(4))) const char* karg_ptr;
    typedef __attribute__((address_space(4))) const T* typed_ptr;
    // The BASE POINTER is made opaque (an empty asm tied to the step's opaque zero), the member's offset stays an immediate of
    // the scalar load (adding `opaque_zero * alignof(T)` to the address cost five scalar instructions per re-read).
    karg_ptr base = (karg_ptr)__builtin_amdgcn_kernarg_segment_ptr();
    asm volatile("" : "+s"(base) : "s"(opaque_zero));
    return *(typed_ptr)(base + byte_off);
#else
    T v;
    __builtin_memset(&v, 0, sizeof(T));
    return v;
#endif
}

// a zero the compiler cannot see through: what depends on it (a kernarg re-read, an address) is evaluated where it stands, not
// hoisted out of the step loop
__device__ __forceinline__ int opaque_zero() {
    int z;
    asm volatile("s_mov_b32 %0, 0" : "=s"(z));
    return z;
}

// base of atc_state_t.phi_wide on the rare paths that need it: the named argument in single-step launches, a kernarg re-read in
// multi-step ones (like the per-episode record's base: nothing about it is carried across the step loop)
template <bool ONE>
__device__ __forceinline__ double* wide_base(double* named, int zk) {
    return ONE ? named : kernarg_reread<double*>(offsetof(StepArgs, st) + offsetof(atc_state_t, phi_wide), zk);
}
// WIDE headings (include/atc_step.h, ABI 19) exist only in wavefronts that are not `plain`; their wrapped counts and observation
// word 3 were left in word 2 of the side record by the first half of this step (step_part_a) — 4-byte loads behind a second
// wave-uniform test, no arithmetic and as few registers as possible where the observation's registers are all live.
// WORD 0: the wrapped counts (what kinematics and angles use in place of phi_fix), WORD 1: observation word 3 as a bit pattern.
template <bool ONE, int WORD>
__device__ __forceinline__ int wide_view(bool plain, int phi, double* named, int zk, uint32_t i, int dflt) {
    int r = dflt;
    if (ATC_RARE(!plain)) {
        if ((__builtin_amdgcn_ballot_w64(phi == INT32_MAX) | __builtin_amdgcn_ballot_w64(phi == INT32_MIN)) != 0ull) {
            if (is_wide(phi)) r = *at<int>(wide_base<ONE>(named, zk), i * 32u + (16u + 4u * WORD));   // (B N 40 < 4 GiB is guaranteed)
            // The load is WAITED FOR here, inside the rare block: left pending, the join below would carry "r may be in flight" into
            // the step's straight line, where the first use of r waits for every earlier vector load as well (one counter, in
            // order) — e.g. the lookup-cell records requested ahead of the observation arithmetic that is meant to cover them.
            asm volatile("" : "+v"(r));
        }
    }
    return r;
}
// Latency-bound instantiation: ONE look-up per step (both words, kept in the vector registers it has to spare) instead of one
// wave-uniform test per use site — a not-taken scalar branch is ~20 cycles of a lone wavefront's chain.
struct WideWords {
    int counts, obs_bits;
};
template <bool ONE>
__device__ __forceinline__ WideWords wide_words(bool plain, int phi, double* named, int zk, uint32_t i) {
    WideWords w = {phi, __float_as_int(phi_real(phi))};
    if (ATC_RARE(!plain)) {
        if ((__builtin_amdgcn_ballot_w64(phi == INT32_MAX) | __builtin_amdgcn_ballot_w64(phi == INT32_MIN)) != 0ull) {
            if (is_wide(phi)) {
                const int2 v = *at<int2>(wide_base<ONE>(named, zk), i * 32u + 16u);
                w.counts = v.x;
                w.obs_bits = v.y;
            }
            asm volatile("" : "+v"(w.counts), "+v"(w.obs_bits));   // (waited for here, inside the rare block: see wide_view)
        }
    }
    return w;
}
// the heading's counts as kinematics and angles see them (both are periodic in the heading)
template <bool ONE>
__device__ __forceinline__ int heading_counts(bool plain, int phi, double* named, int zk, uint32_t i) {
    return wide_view<ONE, 0>(plain, phi, named, zk, i, phi);
}

struct StepOut {        // per-step output bases (uniform pointers)
    float* obs;
    uint16_t* flags;
    float* reward;
    uint8_t* done;
    float *raw_obs, *ac_reward, *min_sep, *term_obs;
    uint32_t* packet;
#if ATC_TRACE
    unsigned long long* trace;   // this step's row of stamps (k_step only: the other kernels leave it out of their initialiser, i.e. null)
#endif
};

// ALLV ("all valid"): the launch's slots are all aircraft — N == W and B * W a multiple of the workgroup size (every BASELINE
// configuration) — so the validity flags are compile-time true: no clamped indices, no validity terms in the active masks, no
// exec-mask regions around the stores, the full-wavefront observation store unconditionally.  Fused 65 536 x 16: 11.9 vs 12.3 us
// per step, 8 192 x 16 2.55 vs 2.70 (r04, same box).  Chosen by the host per launch; other shapes take the general kernels.
template <int W, bool ALLV>
__device__ __forceinline__ LaneIds make_ids(uint32_t slot0, int B, int N) {
    LaneIds d;
    d.tid = threadIdx.x;
    d.lane = d.tid & 63;
    d.slot0 = slot0;
    const uint32_t slots = (uint32_t)B * (uint32_t)W;
    const uint32_t slot = slot0 + d.tid;
    d.k = (int)(slot % W);
    if (ALLV) {
        d.env_valid = d.lane_valid = d.wave_full = true;
        d.e = (int)(slot / W);
        d.i = slot;   // N == W: env * N + k
        return d;
    }
    d.env_valid = slot < slots;
    d.e = d.env_valid ? (int)(slot / W) : B - 1;  // clamped: loads stay in bounds, results are never stored
    d.lane_valid = d.env_valid && d.k < N;
    d.i = d.lane_valid ? (uint32_t)d.e * (uint32_t)N + (uint32_t)d.k : (uint32_t)B * (uint32_t)N - 1u;
    d.wave_full = (N == W) && (slot0 + (uint32_t)(d.tid | 63) < slots);
    return d;
}

// _denormalized_action (atc_gym.py:318-335): action -> (v, h, phi) targets in the state's formats with the host-evaluated
// (multiplier, offset) pairs of derive().  Speed and heading: ONE float64 fma and the saturating, truncating conversion of the
// hardware (NaN -> 0) — the spec of include/atc_step.h.  Altitude (ABI 20): the reference's float64 target itself, a * m + c as one
// fma (altitude_target: evaluated where the step uses it).
__device__ __forceinline__ double altitude_target(const QRates& q, float a) { return __builtin_fma((double)a, q.dec_mh, q.dec_ch); }
__device__ __forceinline__ Targets decode_targets(const QRates& q, const Float3& act) {
    Targets t;
    t.v = cvt_u32_f64(__builtin_fma((double)act.a, q.dec_mv, q.dec_cv));
    t.ah = act.b;
    t.p = cvt_i32_f64(__builtin_fma((double)act.c, q.dec_mp, q.dec_cp));
    return t;
}
// Airplane.action_h (model.py:95-102): h + max(min(target - h, 15 dt), -41 dt) in float64, the reference's operations in its order
__device__ __forceinline__ double altitude_move(double h, double target, double dh_lo, double dh_hi) {
    return h + __builtin_fmax(__builtin_fmin(target - h, dh_hi), dh_lo);
}
// max(min(d, r), -r) for integer differences (the symmetric rate limits of speed and heading)
__device__ __forceinline__ int clamp_sym(int d, int r) { return max(min(d, r), -r); }
// |d| < D for a wrapped 32-bit difference d (atc_gym.py:305-306 on counts): one addition and one unsigned compare
__device__ __forceinline__ bool within(int d, int D) { return (uint32_t)d + (uint32_t)(D - 1) < (uint32_t)(2 * D - 1); }

// ---- first half of AtcGym.step: timestep, rate limits towards the targets, kinematics, MVA floor ---------------------
// RO ("read only", the look-ahead kernel: csrc/atc_lookahead.inc): every store to atc_state_t on the step path is compiled out — here
// the side-record stores of WIDE headings.  Default off: every other instantiation is what it was.
// NB ("named bases", the branch kernel: csrc/atc_branch.inc): the phi_wide and stats bases are the ones the caller hands in, as in a
// single-step launch, while everything else keeps the multi-step form.  A kernarg re-read cannot carry a base that differs per
// candidate.  Default = ONE: every other instantiation is what it was.
template <bool ONE, bool LAT, bool LDSG = false, bool RO = false, bool NB = ONE>
__device__ __forceinline__ Mid step_part_a(const float* __restrict__ grid, const QRates& q, const QKin& qk, const QGrid& qg,
                                           const LaneIds& d, uint32_t tv, double th, int tp, float act_p, LaneState& ls, EnvState& es,
                                           bool repeated, bool all_active, double* wide_named, int zk,
                                           uint64_t& refused_blk, bool refused_known ATC_TRACE_PARAM,
                                           const char* ltab = nullptr, const LdsTab* lt = nullptr) {
    Mid m;
    Aircraft& a = ls.a;
    // `repeated` (wave-uniform): this step repeats the previous step's actions and no env of the wavefront was reset in
    // between — last_action == the accepted targets, so nothing can be counted or changed (see ATC_M_ACTIONS_HELD)
    const bool book = !repeated;
    es.t += 1;  // atc_gym.py:135
    // all_active (wave-uniform, multi-step launches): the caller knows that every lane's aircraft is under control — the masks
    // only change in steps that end an episode or hand an aircraft over — and the per-lane bit test is skipped
    const bool active = all_active ||
                        (d.lane_valid && ((d.k < 32 ? ((uint32_t)es.amask >> d.k) : ((uint32_t)(es.amask >> 32) >> (d.k - 32))) & 1u));
    uint32_t fl = 0;
    float r = q.r_base;  // -0.05 * dt, atc_gym.py:137
    int acts = 0;
    // ---- _action_with_reward x3 (atc_gym.py:139-141,299-335) -> Airplane.action_* (model.py:60-120) ------------------
    // invalid target -> ValueError -> -1 reward, nothing applied, last_action kept (atc_gym.py:303-315); valid -> rate-limited
    // move, actions_taken++ unless |target - last| < discriminator.
    // Speed and heading are 32-bit fixed point (include/atc_step.h): the move is integer arithmetic — exact, like the
    // reference's float64 — with wrapping differences for the speed (valid speeds and the initial last_action 0 are less than
    // 2^31 counts apart) and saturating ones for the heading (its targets are not validated: any action is accepted).
    // (model.py:91-94: float64 compares with the float64 target — written so that a NaN target, the altitude action NaN, is REFUSED like
    // a NaN speed target (include/atc_step.h "Non-finite actions"): accepted iff h_min <= target <= h_max)
    constexpr double h_min = kHMin, h_max = kHMax;
    const bool valid_v = !(tv < kVMinFix || tv > kVMaxFix);
    const bool h_low = !(th >= h_min), h_high = !(th <= h_max);   // (both true for NaN; the same two compares feed `refused` below)
    const bool valid_h = !(h_low || h_high);
    // `plain` (wave-uniform): every lane of the wavefront flies an aircraft under control towards valid targets — the normal
    // case by far (a refused target or a handed-over aircraft in 64 is the exception).  Then nothing is conditional: no
    // select per state component, no refusal penalties, no flag bits.  Otherwise the branch-free general form below.  Both
    // evaluate the same expressions on the lanes they share.
    // (one lane mask per COMPARE, combined on the scalar unit: the ballot of a compound predicate is materialised per lane and
    // compared again — two vector operations per site)
    // ... and a heading target beyond the 32-bit range (the saturated conversion, include/atc_step.h ABI 19) takes the general
    // form too, like a lane whose heading or last heading target is WIDE already (`all_active` vouches that none is)
    // (the latency-bound multi-step instantiation carries this mask across the steps of a held action block: the targets do not
    // change inside one — six compares and five scalar ORs fewer on a lone wavefront's chain)
    uint64_t refused = refused_blk;
    if (!refused_known) {
        refused = __builtin_amdgcn_ballot_w64(tv < kVMinFix) | __builtin_amdgcn_ballot_w64(tv > kVMaxFix) |
                  __builtin_amdgcn_ballot_w64(h_low) | __builtin_amdgcn_ballot_w64(h_high) |
                  (__builtin_amdgcn_ballot_w64(tp == INT32_MAX) | __builtin_amdgcn_ballot_w64(tp == INT32_MIN));
        refused_blk = refused;
    }
    uint64_t special = refused;
    if (!all_active) {
        const int hi = book ? max(a.phi, ls.la_p) : a.phi, lo = book ? min(a.phi, ls.la_p) : a.phi;
        special |= __builtin_amdgcn_ballot_w64(!active) | __builtin_amdgcn_ballot_w64(hi == INT32_MAX) | __builtin_amdgcn_ballot_w64(lo == INT32_MIN);
    }
    const bool plain = special == 0ull;
    int phi_k;   // the heading as the kinematics see it (a WIDE heading wrapped: they are periodic)
    static_assert(kAMin == -kAMax && kPhiDotMin == -kPhiDotMax, "symmetric rate limits assumed (one count limit each)");
    if (ATC_USUAL(plain)) {
        a.v = a.v + (uint32_t)clamp_sym((int)(tv - a.v), q.rate_v);
        a.h = altitude_move(a.h, th, q.dh_lo, q.dh_hi);
        a.phi = a.phi + clamp_sym(sat_sub(tp, a.phi), q.rate_p);
        phi_k = a.phi;
        if (book) {
            acts = (!within((int)(tv - ls.la_v), kDiscrVFix) ? 1 : 0) + (!(__builtin_fabs(th - ls.la_h) < (double)kDiscrH) ? 1 : 0) +
                   (!within(sat_sub(tp, ls.la_p), kDiscrPhiFix) ? 1 : 0);
            ls.la_changed = ls.la_changed || tv != ls.la_v || th != ls.la_h || tp != ls.la_p;
            ls.la_v = tv;
            ls.la_h = th;
            ls.la_p = tp;
        }
    } else {
        {
            const bool valid = valid_v;
            const bool ok = valid && active;
            a.v = ok ? a.v + (uint32_t)clamp_sym((int)(tv - a.v), q.rate_v) : a.v;
            if (book) {
                acts += (ok && !within((int)(tv - ls.la_v), kDiscrVFix)) ? 1 : 0;
                ls.la_changed = ls.la_changed || (ok && tv != ls.la_v);
                ls.la_v = ok ? tv : ls.la_v;
            }
            r = valid ? r : r - 1.0f;
            fl |= valid ? 0u : (uint32_t)ATC_F_INVALID_V;
        }
        {
            const bool valid = valid_h;
            const bool ok = valid && active;
            const double h_new = altitude_move(a.h, th, q.dh_lo, q.dh_hi);
            a.h = ok ? h_new : a.h;
            if (book) {
                acts += (ok && !(__builtin_fabs(th - ls.la_h) < (double)kDiscrH)) ? 1 : 0;
                ls.la_changed = ls.la_changed || (ok && th != ls.la_h);
                ls.la_h = ok ? th : ls.la_h;
            }
            r = valid ? r : r - 1.0f;
            fl |= valid ? 0u : (uint32_t)ATC_F_INVALID_H;
        }
        {
            // heading (model.py:104-120: no validation, no wrap).  The 32-bit saturating form is exact while heading, target and last
            // target are inside the 32-bit range; lanes where one is not redo the move in 64-bit counts with the side array
            // (include/atc_step.h, ABI 19) — in the few wavefronts that hold such a lane.
            const int dd = clamp_sym(sat_sub(tp, a.phi), q.rate_p);
            int phi_new = active ? a.phi + dd : a.phi;
            bool counted = active && !within(sat_sub(tp, ls.la_p), kDiscrPhiFix);
            int la_new = active ? tp : ls.la_p;
            phi_k = phi_new;
            // (lanes without an aircraft compute on a clamped copy of the batch's last one: they must not write its side record)
            const bool wide = d.lane_valid && (is_wide(tp) || is_wide(a.phi) || (book && is_wide(ls.la_p)));
            if (ATC_RARE(__builtin_amdgcn_ballot_w64(wide) != 0ull)) {
                if (wide) {
                    double* w = at<double>(wide_base<NB>(wide_named, zk), d.i * 32u);
                    bool lim;
                    const double T = phi_target_wide(__builtin_fma((double)act_p, q.dec_mp, q.dec_cp), &lim);
                    const double P = is_wide(a.phi) ? w[0] : (double)a.phi;
                    const double rate = (double)q.rate_p;
                    // (a handed-over aircraft keeps its heading; its views are refreshed all the same: they are scratch)
                    const double Pn = active ? P + __builtin_fmin(__builtin_fmax(T - P, -rate), rate) : P;
                    phi_new = cvt_i32_f64(Pn);   // saturating: sat32
                    phi_k = phi_new;
                    if (is_wide(phi_new)) {   // the exact counts, and their views for the rest of this step (wide_view)
                        phi_k = phi_wrap(Pn);
                        if (!RO) {
                            w[0] = Pn;
                            *reinterpret_cast<int2*>(w + 2) = make_int2(phi_k, __float_as_int(phi_obs_wide(Pn)));
                        }
                    }
                    if (book && active) {
                        const double L = is_wide(ls.la_p) ? w[1] : (double)ls.la_p;
                        counted = !(__builtin_fabs(T - L) < (double)kDiscrPhiFix);
                        la_new = cvt_i32_f64(T);
                        if (!RO && is_wide(la_new)) w[1] = T;
                    }
                    fl |= (lim && active) ? (uint32_t)ATC_F_PHI_LIMIT : 0u;
                }
            }
            a.phi = phi_new;
            if (book) {
                acts += counted ? 1 : 0;
                ls.la_changed = ls.la_changed || (active && la_new != ls.la_p);
                ls.la_p = la_new;
            }
        }
    }
    ATC_STAMP_TOP(trace_row, 2);
    // ---- Airplane.step (model.py:122-129): rot_matrix(phi) . [0, (v/3600) dt], float64 from the fixed-point state -----------
    // (an aircraft that is not under control does not move: zero speed -> zero displacement -> floor(0 + dither) = 0 counts)
    uint32_t v_move = a.v;
    if (!plain) {
        v_move = active ? a.v : 0u;
        asm("" : "+v"(v_move));   // (keeps the select on the 32-bit counts: the compiler moved it behind the conversion, onto both halves of the double)
    }
    // (the kinematics are periodic in the heading: a WIDE one goes in wrapped — read back from the side record's scratch word)
    advance<LAT>(qk, phi_k, v_move, es.t, a.x, a.y);
    ATC_STAMP_TOP(trace_row, 3);
    m.x32 = pos_to_real(q.pos_neg_k, qg.pos_x0, a.x);
    m.y32 = pos_to_real(q.pos_neg_k, qg.pos_y0, a.y);
    // MVA floor, first half: only ISSUE the lookup-cell gather here; nothing until the override chain needs its result
    m.lc = LdsCode{0u, 0u};
    if (LDSG) {
        m.cell.cell = make_float2(0.0f, 0.0f);
        m.lc = lds_cell_load(ltab, *lt, m.x32, m.y32);   // (LDS: no vector-memory operation on the step's chain)
    } else {
        m.cell = mva_cell_load(grid, qg.gh, m.x32, m.y32);
    }
    m.active = active;
    m.r = r;
    m.fl = fl;
    m.acts = acts;
    m.repeated = repeated;
    m.plain = plain;
    ATC_STAMP_TOP(trace_row, 4);
    return m;
}

// Extension (README.md:62): noise-abatement areas the aircraft is inside of and below the ceiling of — ATC_F_NOISE plus one
// bit per area in bits 16.. (consumed by the reward stage).  Evaluated while the lookup-grid cell is at hand: the cell names
// the areas whose bounds meet it, and almost every wavefront has no candidate at all.
__device__ __forceinline__ uint32_t noise_areas(const float* __restrict__ K, const float* __restrict__ grid, int n_areas,
                                               const MvaCell& c, float x, float y, double h) {
    const int n_noise = n_areas;
    uint32_t bits = 0;
    if (ATC_RARE(n_noise > 0)) {
        const uint32_t cand = noise_candidates(grid, c);
        if (__builtin_amdgcn_ballot_w64(cand != 0u) != 0ull) {
            for (int q = 0; q < n_noise; ++q) {
                const float* rec = K + (int)K[ATC_H_OFF_POLY] + ((int)K[ATC_H_N_MVA] + q) * ATC_P_WORDS;
                if (((cand >> q) & 1u) && in_bounds(rec, x, y) && h < (double)rec[ATC_P_HEIGHT] &&
                    ray_tracing(x, y, K + (int)rec[ATC_P_VOFF], (int)rec[ATC_P_NVERT]))
                    bits |= (uint32_t)ATC_F_NOISE | (0x10000u << q);
            }
        }
    }
    return bits;
}

// ---- observation store (the end of step_part_b, and k_skip's one store per block): [aircraft][10] rows are 40 B apart, so per-lane
//      stores would scatter 8-byte pieces over 20 cache lines per instruction; a full wavefront instead transposes its 64 x 10
//      block through LDS and writes 2 560 contiguous bytes as 16-byte stores.  Other lanes store their own row.
__device__ __forceinline__ void store_obs_rows(float* obs, const LaneIds& d, const float* o, float* obs_stage) {
    if (ATC_USUAL(d.wave_full)) {
        // addresses from threadIdx itself, not from the lane ids a multi-step launch re-derives through an opaque zero: the
        // compiler then knows the ranges (lane < 64: two of the three row tests fold away, 24-bit multiplies suffice) — with
        // the opaque copies it emitted a quarter-rate 64-bit multiply-add per LDS read
        const uint32_t ln = threadIdx.x & 63u, wv = threadIdx.x >> 6;
        float* tb = obs_stage + __umul24(wv, 64u * ATC_OBS_DIM);
        float2* tb2 = reinterpret_cast<float2*>(tb) + __umul24(ln, ATC_OBS_DIM / 2);   // rows are 40 B: 8-byte aligned
#pragma unroll
        for (int c = 0; c < ATC_OBS_DIM / 2; ++c) tb2[c] = make_float2(o[2 * c], o[2 * c + 1]);
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
        // first aircraft of this wavefront (N == W): wave-uniform, so the multiply runs on the scalar unit
        const uint32_t wave_off = (d.slot0 + (uint32_t)__builtin_amdgcn_readfirstlane((int)(threadIdx.x & ~63u))) * 40u;
        const float4* src = reinterpret_cast<const float4*>(tb);
#pragma unroll
        for (int j = 0; j < 3; ++j) {
            const uint32_t idx = (uint32_t)j * 64u + ln;
            if (idx < 64u * ATC_OBS_DIM / 4u) {
                const float4 v = src[idx];
                float* d4 = at<float>(obs, wave_off + idx * 16u);
                typedef float v4f __attribute__((ext_vector_type(4)));
                __builtin_nontemporal_store(v4f{v.x, v.y, v.z, v.w}, reinterpret_cast<v4f*>(d4));
            }
        }
        __builtin_amdgcn_wave_barrier();
    } else if (d.lane_valid) {
        store_obs(at<float>(obs, times40(d.i)), o);
    }
}

// ---- second half: separation scan, win/timeout, observation, shaping, reductions, outputs, auto-reset --------------
// A by-value kernel argument group where it is needed: the single-step kernel names the argument (the compiler places its
// kernarg load), a multi-step launch re-reads it from the kernarg segment through this step's opaque zero — a scalar load
// inside the step instead of registers held (and spilled to vector-register lanes) across the whole step loop.
#define QGET(member) ((ONE || LAT) ? q.member : kernarg_reread<decltype(q.member)>(offsetof(StepArgs, q) + offsetof(StepDerived, member), zk))

// Separation scan horizon (scan_horizon_limits).  In a multi-step launch of the fast variant a full scan asks its question with
// thresholds no pair can close within the next `horizon` steps and notes which partner batches (four partner distances of the LDS
// scan) hold a pair inside them; the following `horizon` steps scan those batches only, with the exact minima — or nothing at all
// when none was noted.  A 64-aircraft env has no pair inside the thresholds of 6 steps in 66 % of its steps: 4 096 x 64 fused
// 3.8-3.95 vs 5.1-5.3 us per step (DESIGN_HISTORY.md §4).  Ships for the LDS-staged widths only.
#define ATC_SCAN_HORIZON_LDS 6
template <int W, bool FULL, bool ONE>
constexpr int scan_horizon() {
    return (FULL || ONE) ? 0 : (W >= 32 ? ATC_SCAN_HORIZON_LDS : 0);
}
constexpr float kScanHMax = 131072.0f;   // |altitude| below which an altitude step rounds by less than 2^-7 ft (scan_horizon_limits)

// SKIP — the step as the frame-skip kernel (k_skip) runs it: the same arithmetic, state update and auto-reset, but what atc_step
// stores every step (observation, raw observation, flag word, rewards, done, minimum separation) is handed back in registers —
// that kernel accumulates over the block and stores once.  Only the terminal observation is still written here, by the step that
// ends the episode, exactly as atc_step writes it.  FULL means what it means for k_step: an optional output is requested.
struct StepVals {
    float o[ATC_OBS_DIM];      // the observation of this step as atc_step stores it (the raw reset observation on the auto-reset path)
    float zraw[ATC_OBS_DIM];   // FULL: the raw observation (where so.raw_obs is set; zeros otherwise)
    float r, env_r;            // the aircraft's and the env's reward
    float min_d2;              // the env's minimum squared distance (FULL), 1e30 without a pair
    uint32_t fl;
    bool done;
};
// RO: see step_part_a — here the auto-reset path reads the episode number and writes nothing: no per-episode record update, no fences
// around it, no terminal observation.
// NB: see step_part_a — the per-episode record and the side record are addressed from the bases handed in (stp, wide_named).
// TERM_OFF != 0 (k_rollout_policy_ends): the terminal observation is stored without FULL — by the lanes with term_ok set, to row
// `term_row` (in floats) of the array whose pointer lies at byte TERM_OFF of the kernarg segment, read there and then; a NULL stores nothing.
template <int W, bool FULL, bool ONE, bool LAT, bool LDSG = false, bool SKIP = false, bool RO = false, bool NB = ONE, size_t TERM_OFF = 0>
__device__ __forceinline__ bool step_part_b(const float* __restrict__ K, const float* __restrict__ grid,
                                            const atc_params_t& p, const StepDerived& q, const QScan& qs, int zk, int N,
                                            const LaneIds& d, const Mid& m, LaneState& ls,
                                            EnvState& es, const StepOut& so, int32_t* stp, double* wide_named, float4* pos, float* obs_stage,
                                            const float* act_next, Float3& a_next, QRates& qr_next, int& scan_skip, uint32_t& scan_mask,
                                            const char* ltab = nullptr, const LdsTab* lt = nullptr, StepVals* sv = nullptr, size_t term_row = 0,
                                            bool term_ok = false) {
    Aircraft& a = ls.a;
    const bool active = m.active;
    const float x32 = m.x32, y32 = m.y32;
    // the altitude as every value-only formula sees it (glide-path test, shaping terms, separation scan, observation word 2): ONE
    // rounding of the float64 state; the flags that depend on the altitude alone compare the float64 (include/atc_step.h, ABI 20)
    const float hf = (float)a.h;
    float r = m.r;
    uint32_t fl = m.fl;
    int acts = m.acts;
    const int tid = d.tid, lane = d.lane, k = d.k, e = d.e;
    const uint32_t i = d.i;

    // ---- separation scan (extension; README.md:51): 3 nm / 1000 ft among aircraft active at step start ---------------
    // Every lane visits its env's other W-1 slots (never itself); aircraft that are not under control are staged at x = 1e18 so
    // that they neither conflict nor enter the minimum — branch-free.
    // The MVA cell (gather issued in the first half) is resolved AFTER the scan from W = 16 up (the round trip overlaps the scan)
    // and for one-aircraft envs (no scan: observation and shaping terms go first); W = 2 .. 8 resolve before it (the cell in flight
    // across the unrolled xor scan only costs registers).  Edge records per round trip in dirty cells: four for W = 1
    // (latency-bound, registers to spare), two otherwise.  Measurements: DESIGN_HISTORY.md §4, profiles/r03_experiments.txt.
    constexpr int kWalkBatch = (W == 1) ? 4 : ATC_MVA_BATCH;
    constexpr bool kResolveAfterScan = W >= 16 || W == 1;   // (W = 2 .. 8: the unrolled xor scan with the cell in flight costs 4 - 22 registers)
    WideWords ww = {0, 0};
    if (LAT) ww = wide_words<NB>(m.plain, a.phi, wide_named, zk, i);
    float mva = 0.0f;
    int pi = 0;
    if (!kResolveAfterScan) {
        float hgt = 0.0f;
        pi = mva_resolve<kWalkBatch>(K, grid, QGET(g.gh), m.cell, x32, y32, &hgt);
        mva = hgt;   // (0 when outside: mva_resolve leaves the height at 0, atc_gym.py:161)
        fl |= noise_areas(K, grid, qs.n_noise, m.cell, x32, y32, a.h);
    }
    // Multi-step launches: the NEXT step's action is requested here — behind the MVA gathers (loads return in order: issued
    // earlier it would sit in front of them and its HBM latency would be paid at the MVA wait) and with the rest of the
    // step body (scan, corridor, observation, shaping, stores) still ahead to cover it.
    if (ATC_RARE(act_next != nullptr)) a_next = *at<Float3>(act_next, times12(i));
    float min_d2 = 1e30f;
    float margin = 1e30f;  // min over partners of max(d^2 - sep^2, |dh| - sep_ft): conflict iff negative
    // Multi-step launches of the fast variant (scan horizon, see scan_horizon_limits): a FULL scan asks with the horizon thresholds
    // and notes which partner batches hold a pair inside them (`flagged`); for the next kHorizon steps (scan_skip > 0) only those
    // batches can hold a pair that lost its separation — they alone are scanned, with the exact minima, and nothing at all when
    // none was flagged.
    constexpr int kHorizon = SKIP ? 0 : scan_horizon<W, FULL, ONE>();   // (the frame-skip kernel scans in full every step)
    constexpr bool kHZ = kHorizon > 0;
    const ScanLimits lim = {qs.sep2, qs.sep_ft, kHZ ? qs.sep2_h : qs.sep2, kHZ ? qs.sep_ft_h : qs.sep_ft};
    const bool in_horizon = kHZ && scan_skip > 0;             // wave-uniform
    const uint32_t batches = in_horizon ? scan_mask : ~0u;
    if (in_horizon) scan_skip -= 1;
    uint32_t flagged = 0u;
    if (W > 1 && batches != 0u) {
        float xs = x32;
        if (!m.plain) xs = active ? x32 : 1e18f;
        const float sep2 = qs.sep2;
        if (W == 16 && !FULL) {
            int conf = 0;
            NearScan16H<1>::run(xs, y32, hf, sep2, qs.sep_ft, conf);
            margin = conf ? -1.0f : margin;
        } else if (W == 16) {
            PairScan16<1, FULL>::run(xs, y32, hf, sep2, qs.sep_ft, min_d2, margin);
        } else if (W <= 8) {
            pair_scan_xor<W, FULL>(xs, y32, hf, sep2, qs.sep_ft, min_d2, margin);
        } else {
            // W = 32 / 64: partners come from LDS and every unordered pair is evaluated ONCE — lane k visits the partners
            // k + 1 .. k + W/2 (mod W) of its group.  The result reaches the partner as the compare's 64-bit lane mask rotated by
            // the distance inside each group (scalar unit), no return traffic between lanes.  Each group is staged TWICE back to
            // back, one plane per coordinate (x | y | h | d^2 minimum; 8 W floats per group): partner k + d is the float d places
            // after the lane's own whatever k, two neighbouring partners arrive as a register pair (ds_read2_b32) for the packed
            // fp32 instructions (IEEE per component: bit-identical to the scalar forms).  Conflict = (d^2 < sep^2) & (|dh| < sep_ft),
            // the oracle's expression: two compares per pair, masks anded on the scalar unit — 4.5 VALU per pair.
            typedef float v2f __attribute__((ext_vector_type(2)));
            const int gbase = tid & ~(W - 1);
            constexpr int P = 2 * W;                   // floats per plane of a group
            float* own = reinterpret_cast<float*>(pos) + 8 * gbase + k;
            own[0] = xs;          own[W] = xs;
            own[P] = y32;         own[P + W] = y32;
            own[2 * P] = hf;      own[2 * P + W] = hf;
            if (FULL) { own[3 * P] = 1e36f; own[3 * P + W] = 1e36f; }
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
            __builtin_amdgcn_wave_barrier();
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
            constexpr int H = W / 2;   // distances 1 .. H
            constexpr int U = 4;       // partners per LDS batch
            // A lost separation is RARE (it ends the episode): the four compare masks of an LDS batch are only ored into one
            // "anything?" word on the common path; the rotations run behind a wave-uniform test in the few batches that found a pair.
            uint64_t hit = 0;
            const v2f xs2 = {xs, xs}, ys2 = {y32, y32}, hs2 = {hf, hf};
            const float sep_ft = qs.sep_ft;
            // thresholds of this scan: the horizon's in a full scan, the minima themselves inside a horizon (and where there is none)
            const float t2 = in_horizon ? lim.sep2 : lim.sep2_h, tf = in_horizon ? lim.sep_ft : lim.sep_ft_h;
#pragma unroll 1   // (fully unrolled, the 2 H compare masks stay live together: 140-220 spilled SGPRs)
            for (int d0 = H - U + 1; d0 >= 1; d0 -= U) {
                const int batch = (d0 - 1) / U;   // partners d0 .. d0 + U - 1
                if (kHZ && !((batches >> batch) & 1u)) continue;   // wave-uniform: nobody inside the thresholds when the horizon began
                v2f qx[U / 2], qy[U / 2], qh[U / 2];
#pragma unroll
                for (int u = 0; u < U / 2; ++u) {
                    const float* q0 = own + d0 + 2 * u;
                    qx[u] = v2f{q0[0], q0[1]};
                    qy[u] = v2f{q0[P], q0[P + 1]};
                    qh[u] = v2f{q0[2 * P], q0[2 * P + 1]};
                }
                uint64_t mk[U];   // mk[2 u + w]: distance d0 + 2 u + w
                v2f d2k[U / 2], dhk[U / 2];   // (kHZ: kept for the exact question behind the wave-uniform test)
#pragma unroll
                for (int u = U / 2 - 1; u >= 0; --u) {
                    const v2f dx = xs2 - qx[u], dy = ys2 - qy[u];
                    const v2f d2 = __builtin_elementwise_fma(dx, dx, dy * dy);
                    d2k[u] = d2;
                    {
                        const v2f dh = hs2 - qh[u];
                        dhk[u] = dh;
                        // (two ballots anded as scalars: the compare masks themselves — a ballot of the anded predicate is
                        // materialised per lane and compared again)
                        // kHZ: the horizon thresholds (scan_horizon_limits) — a superset of the pairs that lost their separation
                        mk[2 * u] = __builtin_amdgcn_ballot_w64(d2[0] < t2) & __builtin_amdgcn_ballot_w64(fabsf(dh[0]) < tf);
                        mk[2 * u + 1] = __builtin_amdgcn_ballot_w64(d2[1] < t2) & __builtin_amdgcn_ballot_w64(fabsf(dh[1]) < tf);
                    }
                    if (FULL) {   // diagnostic minimum separation: the partner needs the VALUE -> LDS float minimum
#pragma unroll
                        for (int w = 1; w >= 0; --w) {
                            const int dd = d0 + 2 * u + w;   // uniform (H is a multiple of U: no tail)
                            min_d2 = fminf(min_d2, d2[w]);
                            // d^2 >= 0: the IEEE order of non-negative floats is the order of their bit patterns
                            atomicMin(reinterpret_cast<unsigned int*>(own - k + 3 * P + ((k + dd) & (W - 1))), __float_as_uint(d2[w]));
                        }
                    }
                }
                uint64_t any = mk[0];
#pragma unroll
                for (int j = 1; j < U; ++j) any |= mk[j];
                if (ATC_RARE(any != 0ull)) {   // some pair of this batch is inside the thresholds
                    if (kHZ && !in_horizon) {   // ... the horizon's: the batch stays on the list; now the exact question for it
                        flagged |= 1u << batch;
                        any = 0ull;
#pragma unroll
                        for (int j = 0; j < U; ++j) {
                            mk[j] = __builtin_amdgcn_ballot_w64(d2k[j / 2][j % 2] < sep2) & __builtin_amdgcn_ballot_w64(fabsf(dhk[j / 2][j % 2]) < sep_ft);
                            any |= mk[j];
                        }
                    }
                    // a pair that lost its separation: both of its lanes are marked
                    hit |= any;
#pragma unroll
                    for (int j = 0; j < U; ++j) {
                        const int dd = d0 + j;   // 1 .. W / 2, uniform
                        const uint64_t t = mk[j];
                        if (W == 64) {
                            hit |= (t << dd) | (t >> (64 - dd));
                        } else {  // two groups of 32 lanes: rotate inside each half
                            const uint32_t lo = (uint32_t)t, hi = (uint32_t)(t >> 32);
                            hit |= (uint64_t)((lo << dd) | (lo >> (32 - dd))) | ((uint64_t)((hi << dd) | (hi >> (32 - dd))) << 32);
                        }
                    }
                }
            }
            if ((hit >> lane) & 1ull) margin = -1.0f;
            if (FULL) {
                __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
                __builtin_amdgcn_wave_barrier();
                __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
                min_d2 = fminf(min_d2, own[3 * P]);
            }
            __builtin_amdgcn_wave_barrier();
        }
        if (kHZ && !in_horizon) {
            // the horizon's premises (scan_horizon_limits): no aircraft faster than 300 kt, altitudes of ordinary magnitude (a NaN fails)
            const uint64_t odd = __builtin_amdgcn_ballot_w64(a.v > kVMaxFix) | __builtin_amdgcn_ballot_w64(!(fabsf(hf) < kScanHMax));
            scan_skip = (odd != 0ull) ? 0 : kHorizon;
            scan_mask = flagged;
        }
    }
    ATC_STAMP_B(2);
    Obs ob;
    float shaping = 0.0f;
    const ObsConst oc = QGET(oc);
    // (W = 1 has no scan to cover the gather: there the observation goes first)
    // A dirty cell's first record (the LINE record of a split cell) is requested BEFORE the observation arithmetic, which then comes
    // before the resolve: the lookup's second dependent L2 trip overlaps ~100 instructions instead of stalling the wavefront.
    // Measured per width and launch form (r04, same box, two rounds): single steps of 16-aircraft envs 17.81 vs 18.03 us at
    // 65 536 envs, one-aircraft envs 6.58-6.61 vs 6.60-6.67 single / 3.42 vs 3.47-3.50 fused; NOT the fused 16-aircraft launch
    // (8 B scratch under its 80-register bound: 2.73-2.77 vs 2.66 us at 8 192 envs) and not the 64-aircraft kernels (8.50 vs 8.30).
    constexpr bool kPrefetch = (W == 1 || (ONE && W == 16)) && kResolveAfterScan && !LDSG;
    constexpr bool kObsFirst = kPrefetch || W == 1;
    MvaPre pre;
    if (kPrefetch) pre = mva_prefetch(grid, QGET(g.gh), m.cell);
    if (kObsFirst) {
        // (observation word 3 first, then the heading for the angles — each its own rare look-up for a WIDE heading, before the rest
        // of the observation occupies its registers)
        const WideWords wo = LAT ? ww : wide_words<NB>(m.plain, a.phi, wide_named, zk, i);   // (ONE test for both words)
        const float phi_f = phi_real(wo.counts), phi_o = __int_as_float(wo.obs_bits);
        ob = get_state(oc, a.x, a.y, x32, y32, hf, phi_f, phi_o, v_real(a.v), hf);   // (word 5 = h - mva follows the resolve)
        if (p.mode & ATC_M_REWARD_SHAPING) shaping = shaping_total(shaping_core(oc, ob.d_faf, ob.phi_rel_faf, ob.o[9], hf, ob.on_gp));
    }
    ATC_STAMP_TOP(so.trace, 5);
    // ---- MVA floor (atc_gym.py:146-161), second half ---------------------------------------------------------------------
    if (LDSG) {
        // the LDS-resident table (csrc/atc_device.h: lds_resolve); the host attaches one only to sectors without noise-abatement areas
        float hgt = 0.0f;
        uint32_t walk;
        bool band;
        pi = lds_resolve(ltab, *lt, m.lc, x32, y32, &hgt, &walk, &band);
        if (ATC_RARE(__builtin_amdgcn_ballot_w64(walk != 0u) != 0ull)) {   // a vertex sub-cell: those lanes walk its records (one trip)
            if (walk != 0u) pi = lds_walk(*lt, walk, x32, y32, &hgt);
            asm volatile("" : "+v"(pi), "+v"(hgt));   // (waited for inside the rare block: see wide_view)
        }
        if (ATC_RARE(__builtin_amdgcn_ballot_w64(band) != 0ull)) {   // inside a line's margin band: the wavefront asks the grid
            const GridHdr gh = QGET(g.gh);
            const MvaCell c = mva_cell_load(grid, gh, x32, y32);
            pi = mva_resolve<kWalkBatch>(K, grid, gh, c, x32, y32, &hgt);
            asm volatile("" : "+v"(pi), "+v"(hgt));
        }
        mva = hgt;
    } else if (kResolveAfterScan) {
        float hgt = 0.0f;
        pi = mva_resolve<kWalkBatch>(K, grid, QGET(g.gh), m.cell, x32, y32, &hgt, kPrefetch ? &pre : nullptr);
        mva = hgt;                                 // atc_gym.py:161: mva = 0 outside (mva_resolve leaves the height at 0)
        fl |= noise_areas(K, grid, qs.n_noise, m.cell, x32, y32, a.h);
    }
    ATC_STAMP_END(so.trace, 1);
    // ---- the override chain (atc_gym.py:146-173) -----------------------------------------------------------------------
    // `quiet` (wave-uniform): nothing of it applies to any lane of this wavefront — every aircraft under control with accepted
    // targets (plain), inside the airspace at or above its MVA, no separation lost, no time-out, outside the bounds of the
    // corridor's horizontal triangle (the exact early-out of Runway.inside_corridor; asked of the lookup cell, which carries a
    // candidate bit), in no noise-abatement area.  That is
    // what almost every step of almost every wavefront looks like, and then reward and flag word are what the first half left
    // (base reward, no flag): the chain's selects run only in the other wavefronts — the same expressions, lane for lane.
    const bool conflict = margin < 0.0f;
    const bool timeout = es.t > qs.timestep_limit;
    // (one lane mask per compare, combined on the scalar unit — see `plain`)
    const uint64_t in_tri = LDSG ? __builtin_amdgcn_ballot_w64(lds_corridor_candidate(m.lc))
                          : grid ? __builtin_amdgcn_ballot_w64(corridor_candidate(m.cell))
                                 : (__builtin_amdgcn_ballot_w64(x32 >= qs.tri_bbox.x) & __builtin_amdgcn_ballot_w64(x32 <= qs.tri_bbox.z) &
                                    __builtin_amdgcn_ballot_w64(y32 >= qs.tri_bbox.y) & __builtin_amdgcn_ballot_w64(y32 <= qs.tri_bbox.w));
    const double mva_d = (double)mva;   // (an integer height; 0 outside the airspace)
    const bool quiet = m.plain &&
                       (__builtin_amdgcn_ballot_w64(pi < 0) | __builtin_amdgcn_ballot_w64(a.h < mva_d) | __builtin_amdgcn_ballot_w64(margin < 0.0f) |
                        __builtin_amdgcn_ballot_w64(es.t > qs.timestep_limit) | __builtin_amdgcn_ballot_w64(fl > 0xffffu) | in_tri) == 0ull;
    if (ATC_RARE(!quiet)) {
        {
            const bool below = pi >= 0 && a.h < mva_d;   // atc_gym.py:149: float64 altitude against the integer height
            r = pi < 0 ? -50.0f : (below ? -200.0f : r);
            fl |= pi < 0 ? (uint32_t)ATC_F_OUTSIDE : (below ? (uint32_t)ATC_F_BELOW_MVA : 0u);
        }
        {   // conflict override comes after the MVA overrides in the chain
            r = conflict ? qs.conflict_reward : r;
            fl |= conflict ? (uint32_t)ATC_F_CONFLICT : 0u;
        }
        // ---- win / timeout overrides (atc_gym.py:163-173) ---------------------------------------------------------------
        if (inside_corridor(K, qs.tri_bbox, x32, y32, hf, (double)(LAT ? ww.counts : heading_counts<NB>(m.plain, a.phi, wide_named, zk, i)))) {
            int bonus = (qs.timestep_limit - es.t) * 5;
            bonus = bonus < 0 ? 0 : bonus;
            r = (float)(10000 + bonus);
            fl |= ATC_F_WON;
        }
        {
            r = timeout ? -200.0f : r;
            fl |= timeout ? (uint32_t)ATC_F_TIMEOUT : 0u;
        }
    }
    ATC_STAMP_B(3);
    ATC_STAMP_END(so.trace, 2);
    // ---- observation, shaping, noise areas, normalisation (atc_gym.py:175-189) ------------------------------------------
    // (multi-step launches: the normalisation constants are requested here, a hundred vector operations ahead of their use —
    // requested where they are used, the scalar load's whole latency was a stall)
    const QNorm qn = QGET(n);
    float o[ATC_OBS_DIM];
    float zraw[ATC_OBS_DIM];   // FULL only: raw observation (zeros for handed-over aircraft)
    {
        if (kObsFirst) {
            ob.o[5] = alt_above(a.h, mva);
        } else {
            const WideWords wo = LAT ? ww : wide_words<NB>(m.plain, a.phi, wide_named, zk, i);
            const float phi_f = phi_real(wo.counts), phi_o = __int_as_float(wo.obs_bits);
            ob = get_state(oc, a.x, a.y, x32, y32, hf, phi_f, phi_o, v_real(a.v), alt_above(a.h, mva));
            if (p.mode & ATC_M_REWARD_SHAPING) shaping = shaping_total(shaping_core(oc, ob.d_faf, ob.phi_rel_faf, ob.o[9], hf, ob.on_gp));
        }
        // r += pos; r += ang; r += gs (atc_gym.py:179-185, after the override chain) as one addition of the factored sum
        // (value-only, within 1e-5)
        if (p.mode & ATC_M_REWARD_SHAPING) r += shaping;
        // extension (README.md:62): noise-abatement areas — which ones the aircraft is in was decided next to the MVA lookup
        // (bits 16.. of fl); the penalties are subtracted here, after the shaping terms, in area order.
        if (ATC_RARE(!quiet && __builtin_amdgcn_ballot_w64((fl >> 16) != 0u) != 0ull)) {
            const int n_noise = qs.n_noise;
            for (int q = 0; q < n_noise; ++q)
                if ((fl >> (16 + q)) & 1u) r -= (K + (int)K[ATC_H_OFF_POLY] + ((int)K[ATC_H_N_MVA] + q) * ATC_P_WORDS)[ATC_P_PENALTY];
            fl &= 0xffffu;
        }
        if (FULL && !SKIP) {
#pragma unroll
            for (int c = 0; c < ATC_OBS_DIM; ++c) zraw[c] = active ? ob.o[c] : 0.0f;  // zeros for handed-over aircraft
            if (so.raw_obs && d.lane_valid) store_obs(at<float>(so.raw_obs, times40(i)), zraw);
        }
        if (FULL && SKIP) {
#pragma unroll
            for (int c = 0; c < ATC_OBS_DIM; ++c) zraw[c] = (so.raw_obs && active) ? ob.o[c] : 0.0f;
        }
        // atc_gym.py:187-189: (s - min - max/2) / (max/2) as one fma; the identity (1, -0) without ATC_M_NORMALIZE (derive())
#pragma unroll
        for (int c = 0; c < ATC_OBS_DIM; ++c) o[c] = fmaf(ob.o[c], qn.a[c], qn.b[c]);
    }
    // lanes without an aircraft under control: nothing happened.  Almost every wavefront has none, so the selects sit
    // behind a wave-uniform test.
    if (ATC_RARE(!m.plain && __builtin_amdgcn_ballot_w64(!active) != 0ull)) {
#pragma unroll
        for (int c = 0; c < ATC_OBS_DIM; ++c) o[c] = active ? o[c] : 0.0f;
        r = active ? r : 0.0f;
        acts = active ? acts : 0;
        fl = active ? fl : (d.lane_valid ? (uint32_t)ATC_F_INACTIVE : 0u);
        if (!active) min_d2 = 1e30f;
    }

    ATC_STAMP_B(4);
    ATC_STAMP_END(so.trace, 3);
    // ---- per-env reductions over the W lanes of the group ----------------------------------------------------------------
    const float env_r = group_sum<W>(r);
    const int env_acts = m.repeated ? 0 : group_sum_i<W>(acts);
    bool done = false, env_won = false;
    if (ATC_RARE(!quiet)) {
        const uint64_t won = group_ballot<W>((fl & ATC_F_WON) != 0, lane);
        const uint64_t term = group_ballot<W>(
            (fl & (ATC_F_BELOW_MVA | ATC_F_OUTSIDE | ATC_F_CONFLICT | ATC_F_TIMEOUT)) != 0, lane);
        // extension: an aircraft that reaches the corridor is handed over; the episode is won when all are.
        // ATC_M_KEEP_ACTIVE: the reference's rule (atc_gym.py:163-169) — any win ends the episode, nobody is handed over.
        const bool keep_active = (p.mode & ATC_M_KEEP_ACTIVE) != 0;
        if (!keep_active) es.amask &= ~won;
        env_won = keep_active ? won != 0 : es.amask == 0;
        done = d.env_valid && (term != 0 || env_won);
        // an env that restarts inside this step puts its aircraft somewhere else: the scan horizon ends here
        if (kHZ && (p.mode & ATC_M_AUTO_RESET) && __builtin_amdgcn_ballot_w64(done) != 0ull) scan_skip = 0;
    }
    es.total_reward += env_r;  // atc_gym.py:194-197
    es.n_actions += env_acts;

    // (flag word, reward and done are stored at the END of the step, behind the observation: see there)
    if (FULL && ONE && W == 1 && so.packet && d.lane_valid) {
        // The step result of a single-aircraft env as 9 self-validating 16-byte chunks (include/atc_step.h, atc_out_t.packet):
        // each chunk is ONE store carrying the caller's sequence tag, so a host polling mapped memory never mixes steps.
        const uint32_t tag = p.reserved0;
        const float w[27] = {o[0], o[1], o[2], o[3], o[4], o[5], o[6], o[7], o[8], o[9], zraw[0], zraw[1], zraw[2], zraw[3],
                             zraw[4], zraw[5], zraw[6], zraw[7], zraw[8], zraw[9], env_r,
                             __uint_as_float((fl & 0xffffu) | (done ? 0x10000u : 0u)), __int_as_float(es.t),
                             __int_as_float(es.n_actions), __int_as_float(a.x), __int_as_float(a.y), 0.0f};
        uint4* pk = at<uint4>(so.packet, (uint32_t)e * (ATC_PKT_CHUNKS * 16u));
#pragma unroll
        for (int c = 0; c < ATC_PKT_CHUNKS; ++c)
            store16_system(pk + c, __float_as_uint(w[3 * c]), __float_as_uint(w[3 * c + 1]), __float_as_uint(w[3 * c + 2]), tag);
    }
    if (SKIP) sv->min_d2 = (FULL && W > 1) ? group_min<W>(min_d2) : 1e30f;
    if (FULL && !SKIP && so.min_sep) {
        const float m2 = (W > 1) ? group_min<W>(min_d2) : 1e30f;
        if (d.env_valid && k == 0) *at<float>(so.min_sep, (uint32_t)e * 4u) = (m2 >= 1e30f) ? 1e30f : sqrtf(m2);
    }

    if (ATC_RARE(done && (p.mode & ATC_M_AUTO_RESET))) {
        // VecEnv semantics: the env restarts inside the step; the returned obs is the RAW reset state
        // (atc_gym.py:351,365: reset() returns the un-normalised state computed with mva = 0).
        // The per-episode record is read, updated and written here and nowhere else on the step path.  In a multi-step launch
        // an earlier step of this wavefront may have written it (lane k == 0 writes, all lanes of the env read): wavefront-
        // scope fences order those accesses (they compile to nothing — a wavefront's memory operations are issued in order).
        if (!RO) __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
        // (multi-step launches fetch the record's base here, on the rare path: carried from the top of the step it sat in
        // vector-register lanes)
        int32_t* stats = NB ? stp : kernarg_reread<int32_t*>(offsetof(StepArgs, st) + offsetof(atc_state_t, stats), zk);
        int4* sr = at<int4>(stats, (uint32_t)e * (ATC_STAT_WORDS * 4u));
        const int4 s0 = sr[0];  // episodes, ep_length, ep_return, win_bits
        const int episode = s0.x;
        if (!RO && d.env_valid && k == 0) {
            const uint32_t win_bits = (((uint32_t)s0.w << 1) | (env_won ? 1u : 0u)) & 0x3ffu;
            sr[0] = make_int4(episode + 1, es.t, __float_as_int(es.total_reward), (int)win_bits);
            *at<int>(stats, (uint32_t)e * (ATC_STAT_WORDS * 4u) + ATC_STAT_EP_ACTIONS * 4u) = es.n_actions;
        }
        if (!RO) __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        if (d.lane_valid) {
            if (!RO && FULL && so.term_obs) store_obs(at<float>(so.term_obs, times40(i)), o);
            if constexpr (TERM_OFF != 0) {
                float* const term_obs = kernarg_reread<float*>(TERM_OFF, zk);
                if (term_obs && term_ok) store_obs(at<float>(term_obs + term_row, times40(i)), o);
            }
            // (slot through this step's opaque zero: the spawn-record address is then formed here, on the rare path, instead of
            // being carried — and spilled — across the step loop as a 64-bit per-lane pointer)
            a = spawn(K, qs.off_spawn, p, e, k + zk, episode, o);   // state + raw reset observation from the blob's spawn records
        }
        es.total_reward = 0.0f;
        es.n_actions = 0;
        es.t = 0;
        es.amask = (N >= 64) ? ~0ull : ((1ull << N) - 1ull);
    }

    ATC_STAMP_B(5);
    ATC_STAMP_END(so.trace, 4);
    // Multi-step launches: the NEXT step's rate group is requested here, with the observation store still ahead — requested at
    // the top of the step that uses it, its latency was a stall before the first instruction of the kinematics.
    if (!ONE && !LAT) qr_next = kernarg_reread<QRates>(offsetof(StepArgs, q) + offsetof(StepDerived, r), opaque_zero());
    // The next block's action (requested above, behind the MVA gathers) is WAITED FOR here, in the step that requested it and ahead
    // of this step's stores: left pending across the loop's back edge, "the action may be in flight" reaches the loop header, and the
    // decode at the top of EVERY step waits for every earlier vector-memory operation — one counter, in order — i.e. for the
    // previous step's observation stores to complete.  By now the load has long arrived.
    if (ATC_RARE(act_next != nullptr)) asm volatile("" : "+v"(a_next.a), "+v"(a_next.b), "+v"(a_next.c));
    if (SKIP) {   // nothing is stored per step: the values go back to k_skip
#pragma unroll
        for (int c = 0; c < ATC_OBS_DIM; ++c) { sv->o[c] = o[c]; sv->zraw[c] = FULL ? zraw[c] : 0.0f; }
        sv->r = r;
        sv->env_r = env_r;
        sv->fl = fl;
        sv->done = done;
        return quiet;
    }
    store_obs_rows(so.obs, d, o, obs_stage);
    ATC_STAMP_END(so.trace, 5);
    // ---- flag word, reward, done: last.  The compiler guards the observation's staging registers with a wait for ALL vector
    //      memory operations (one counter for loads and stores; the auto-reset path's loads merge in above) — issued before the
    //      observation, these three small stores were waited for there, a store round trip in every step.  Here the next such
    //      wait is the lookup-cell gather of the following step, a kinematics stage and a separation scan later.
    if (d.lane_valid) {
        stream_store(at<uint16_t>(so.flags, i * 2u), (uint16_t)fl);
        if (FULL && so.ac_reward) *at<float>(so.ac_reward, i * 4u) = r;
    }
    if (d.env_valid && k == 0) {
        *at<float>(so.reward, (uint32_t)e * 4u) = env_r;
        *at<uint8_t>(so.done, (uint32_t)e) = done ? 1 : 0;
    }
    return quiet;
}

__device__ __forceinline__ void store_lane_state(const atc_state_t& st, const LaneIds& d, const LaneState& ls, bool la_live) {
    if (d.lane_valid) {
        *at<int4>(st.ac, d.i * 16u) = make_int4(ls.a.x, ls.a.y, ls.a.phi, (int)ls.a.v);
        *at<double>(st.alt, d.i * 8u) = ls.a.h;
    }
    // the last-action targets are typically constant for many steps (actions are held): written back only by wavefronts in which
    // one of them changed
    if (__builtin_amdgcn_ballot_w64(ls.la_changed) != 0ull && d.lane_valid && la_live)
        *at<int4>(st.last_act, d.i * 16u) = make_int4((int)ls.la_v, ls.la_p, __double2loint(ls.la_h), __double2hiint(ls.la_h));
}
template <int W>
__device__ __forceinline__ void store_env_state(const atc_state_t& st, const LaneIds& d, const EnvState& es, uint32_t hi0) {
    if (d.env_valid && d.k == 0) {
        *at<int4>(st.env, (uint32_t)d.e * (ATC_ENV_WORDS * 4u)) =
            make_int4(es.t, es.n_actions, __float_as_int(es.total_reward), (int)(uint32_t)(es.amask & 0xffffffffu));
        if (W == 64 && (uint32_t)(es.amask >> 32) != hi0)
            *at<uint32_t>(st.stats, (uint32_t)d.e * (ATC_STAT_WORDS * 4u) + ATC_STAT_MASK_HI * 4u) = (uint32_t)(es.amask >> 32);
    }
}

// Multi-step kernels WAIT for their state loads here, before the step loop.  Left pending, "a state register may still be in flight"
// is merged into the loop header from the pre-header, and the compiler guards the first use of each in the loop body with a wait
// that — one counter for loads and stores, in order — also waits for the PREVIOUS step's stores in every later step.
__device__ __forceinline__ void settle_state(LaneState& ls, EnvState& es) {
    asm volatile("" : "+v"(ls.a.x), "+v"(ls.a.y), "+v"(ls.a.h), "+v"(ls.a.phi), "+v"(ls.a.v));
    asm volatile("" : "+v"(ls.la_v), "+v"(ls.la_h), "+v"(ls.la_p), "+v"(es.t), "+v"(es.n_actions), "+v"(es.total_reward));
    uint32_t m_lo = (uint32_t)es.amask, m_hi = (uint32_t)(es.amask >> 32);
    asm volatile("" : "+v"(m_lo), "+v"(m_hi));
    es.amask = (uint64_t)m_lo | ((uint64_t)m_hi << 32);
}

// Fill-phase prefetch (fast single-step launches of envs of up to 16 aircraft; DESIGN.md section 3, profiles/fill_prefetch_*).  The
// workgroups of the launch's first round — blockIdx.x < pf_stride, the workgroups the device holds at once (host: launch_step2) —
// also touch the ac and alt records of the slot pf_stride workgroups further on: they all wait for their own state together, compute
// together and store together, and until their first stores leave the memory system has nothing to do.  The lines land in the L2 of
// the XCD that will run workgroup blockIdx.x + pf_stride (workgroups are dealt round-robin to the 8 XCDs, pf_stride is a multiple
// of 8), which then finds them there.
//   ONE WORD of each record is requested, not the record: the line comes all the same, and two registers held to the end of the
//   kernel keep the launch at 71 VGPRs = 7 wavefronts per SIMD (whole records: 78 and 6).  The request is unconditional — a
//   workgroup with nothing to prefetch reads the first record of its own tile, one line it has just asked for — because behind a
//   branch the compiler waits for EVERY load at the join, the prefetch included, before the first instruction of the decode.
//   The values are discarded; the empty asm behind the kernel's last stores keeps them alive, so nothing waits for them before the
//   in-order return of the lookup-cell gather does anyway.  Measured variants (action too, half a round, behind the gather, whole
//   records): profiles/experiments/README.md.
// Why it cannot change a result: the records touched are written in this launch by ONE workgroup, the one they belong to, which
// reads them (its own loads) before it writes them — whatever this workgroup sees is thrown away; a line that lands in another
// XCD's L2 than its reader's is never read in this launch, and the next launch starts with the L2 invalidate of every kernel
// boundary (what makes fetched bytes equal algorithmic bytes today).  The index is in bounds: the whole target tile lies below B * N.
#define ATC_FILL_PREFETCH(W, FULL, ONE, ALLV) ((ONE) && !(FULL) && (ALLV) && (W) <= 16)

#define ATC_LAT_WAVES 2   // wavefronts per SIMD the latency-bound instantiation is register-budgeted for (<= 256 VGPRs)
// ONE: single-step launch (T == 1); ALLV: every slot is an aircraft (make_ids); LAT: latency-bound multi-step instantiation (above)
// LDSG: the latency-bound launch of ONE-aircraft envs with the sector's lookup table staged in LDS (csrc/atc_device.h: LdsTab) — one
// workgroup per CU (the table's staged part is 112 KB for LOWW), chosen by the host when the launch has no more workgroups than the device CUs
template <int W, bool FULL, bool ONE, bool ALLV, bool LAT = false, bool LDSG = false>
__global__ void __launch_bounds__(kBlock, (LDSG ? 1 : LAT ? ATC_LAT_WAVES : ONE ? ATC_MIN_WAVES : ((FULL || W <= 8 || W >= 32) ? ATC_MIN_WAVES_LOOP - 1 : ATC_MIN_WAVES_LOOP)))
k_step(const float* __restrict__ blob, int off_grid, int B, int N, int T, int hold, atc_state_t st,
       const float* __restrict__ actions, atc_out_t out, atc_params_t p, StepDerived q_arg, InlineAction ia, LdsTab lt_arg, int pf_stride) {
    static_assert(!LAT || (!ONE && !FULL), "LAT is an instantiation of the fast multi-step kernels");
    static_assert(!LDSG || (LAT && W == 1 && ALLV), "LDSG is an instantiation of the latency-bound one-aircraft kernel");
    StepDerived q_vec;
    if (LAT) q_vec = to_vector_registers(q_arg);
    const StepDerived& q = LAT ? q_vec : q_arg;
    extern __shared__ __attribute__((aligned(16))) float smem[];
    float4* pos = reinterpret_cast<float4*>(smem);                    // [2 kBlock] pair-scan staging (W >= 32)
    float* obs_stage = smem + (W >= 32 ? 2 * kBlock * 4 : 0);  // [4 waves][64 x 10] obs transpose
    const float* __restrict__ K = blob;  // the sector: uniform-index reads -> scalar loads
    const float* __restrict__ grid = off_grid ? blob + off_grid : nullptr;
#if ATC_TRACE
    const int tid = threadIdx.x, lane = tid & 63;
    unsigned long long* trace = reinterpret_cast<unsigned long long*>(
        ((unsigned long long)p.reserved0) | ((unsigned long long)__float_as_uint(p.reserved1) << 32));
    const unsigned long long t_launch = __builtin_amdgcn_s_memtime();
#endif
    const uint32_t BN = (uint32_t)B * (uint32_t)N;      // host guarantees B*N*40 bytes < 4 GiB: 32-bit lane offsets
// single-step launches of envs of up to 16 aircraft (r05, same box: 8 192 x 16 5.15 vs 5.34 us, 65 536 x 16 17.53 vs 17.60, 65 536 x 1
// 6.03 vs 6.13 with the argument preload; 4 096 x 64 8.0 vs 7.8 and the multi-step launches no better: off there)
#define ATC_KARG_PREFETCH(W, ONE) ((ONE) && (W) <= 16)
    int karg_touch = 0;
    if (ATC_KARG_PREFETCH(W, ONE)) {
        // Touch every 64-byte line of the kernarg segment NOW, in one burst of scalar loads: the step reads its ~530 bytes of
        // arguments at a dozen places, each just ahead of its use — in a wavefront that is the first of its dispatch on its scalar
        // cache every one of those is a miss on the step's serial chain; requested together up front the misses overlap and the
        // later reads hit.
#if __HIP_DEVICE_COMPILE__
        typedef __attribute__((address_space(4))) const int* karg_ip;
        karg_ip kb = (karg_ip)__builtin_amdgcn_kernarg_segment_ptr();
#pragma unroll
        for (int ln = 1; ln < (int)((offsetof(StepArgs, lt) + 63) / 64); ++ln) karg_touch ^= kb[16 * ln];   // (lt: read by the LDSG launch only)
#endif
    }
    const LaneIds d = make_ids<W, ALLV>(blockIdx.x * kBlock, B, N);

    // ---- load persistent state (16-byte records; the W lanes of an env share the env record) -------------------------
    const int4 e0 = *at<int4>(st.env, (uint32_t)d.e * (ATC_ENV_WORDS * 4u));
    const uint32_t hi0 = (W == 64) ? *at<uint32_t>(st.stats, (uint32_t)d.e * (ATC_STAT_WORDS * 4u) + ATC_STAT_MASK_HI * 4u) : 0u;
    EnvState es = {e0.x, e0.y, __int_as_float(e0.z), (uint64_t)(uint32_t)e0.w | ((uint64_t)hi0 << 32)};
    const int4 ps = *at<int4>(st.ac, d.i * 16u);       // x, y, heading, speed
    const double h0 = *at<double>(st.alt, d.i * 8u);
    // ATC_M_ACTIONS_HELD (single-step launches): the caller repeats the previous launch's actions, so an aircraft that was under
    // control then has last_action == its accepted targets and cannot count an action or change the record — the 16-byte
    // record is only read (and written) by envs that were reset since their last step (timesteps == 0), whose aircraft
    // may have been handed over when the action block started and still carry an older record.
    Float3 act = {0.0f, 0.0f, 0.0f};   // action of the current block (held for `hold` steps); one 12-byte load per lane
    if (ONE && W == 1 && FULL && ia.set) {   // the single env of atc_step_packet: the action came with the kernel arguments
        act = Float3{ia.v, ia.h, ia.p};
    } else if (ONE) {
        act = *at<Float3>(actions, times12(d.i));   // requested before the env record is waited for below
    }
    const bool same_actions = ONE && (p.mode & ATC_M_ACTIONS_HELD) != 0;
    const bool la_live = !same_actions || e0.x == 0;
    int4 la0 = make_int4(0, 0, 0, 0);   // v, heading, altitude target (float64)
    if (la_live) la0 = *at<int4>(st.last_act, d.i * 16u);
    LaneState ls = {{ps.x, ps.y, h0, ps.z, (uint32_t)ps.w}, (uint32_t)la0.x, __hiloint2double(la0.w, la0.z), la0.y, false};
    int pf_ac = 0, pf_alt = 0;
    if (ATC_FILL_PREFETCH(W, FULL, ONE, ALLV)) {   // (see ATC_FILL_PREFETCH)
        const bool pf_on = blockIdx.x < (uint32_t)pf_stride && (blockIdx.x + (uint32_t)pf_stride) * kBlock < BN;
        const uint32_t pi = pf_on ? d.i + (uint32_t)pf_stride * kBlock : d.slot0;
        pf_ac = *at<int>(st.ac, pi * 16u);
        pf_alt = *at<int>(st.alt, pi * 8u);
    }

    // A single step is its own instantiation: with the step count a run-time value everything the loop carries (aircraft
    // and env records, output bases, hoisted sector constants) stays live across the whole body — the straight-line form
    // needs 56 VGPRs (N = 16), the loop form 80 under its launch bound (94 without it).
    const int n_steps = ONE ? 1 : T;
    const float* act_t = actions;   // action block of the current step; a block is held for `hold` steps
    int left = hold;                // steps the current block is still used for
    bool block_start = true;        // this step is the first of its block
    Targets tg = {0u, 0.0f, 0};   // decoded targets of the current step / block
    uint64_t refused_blk = 0ull;  // LAT: which lanes' speed / altitude / heading targets of the current block are refused or beyond range
    bool refused_known = false;
    bool all_active = false, mask_dirty = true;
    int scan_skip = 0;          // wave-uniform: steps left in the separation scan's horizon (step_part_b) ...
    uint32_t scan_mask = 0u;    // ... and the partner batches that have to be scanned inside it
    QRates qr_next = q.r;   // the rate group of the coming step (multi-step launches fetch it one step ahead, see step_part_b)
    if (!ONE && !LAT) qr_next = kernarg_reread<QRates>(offsetof(StepArgs, q) + offsetof(StepDerived, r), opaque_zero());
    // LDSG: stage the lookup table — 28 sixteen-byte pieces per lane in flight at a time (ONE round trip for LOWW's 112 KB), behind
    // the state loads issued above; the terms a step reads with the table go to vector registers like the other uniform terms (LAT)
    LdsTab ltv = lt_arg;
    const char* ltab = nullptr;
    if (LDSG) {
        uint4* dst = reinterpret_cast<uint4*>(smem + (kBlock / 64) * 64 * ATC_OBS_DIM);   // behind the observation transpose stage
        const int n16 = lt_arg.n16;
        constexpr int kDepth = 28;   // (LOWW: 7 144 pieces = ONE batch of 28 x 256)
        for (int base = 0; base < n16; base += kDepth * kBlock) {
            uint4 v[kDepth];
#pragma unroll
            for (int u = 0; u < kDepth; ++u) {
                const int j = base + u * kBlock + (int)threadIdx.x;
                v[u] = lt_arg.src[min(j, n16 - 1)];
            }
            // (every load is USED here, unconditionally: left to the conditional stores below, the compiler sinks each load into its
            // store's exec-mask region — one round trip per piece instead of one per batch)
#pragma unroll
            for (int u = 0; u < kDepth; ++u) asm volatile("" : "+v"(v[u].x), "+v"(v[u].y), "+v"(v[u].z), "+v"(v[u].w));
#pragma unroll
            for (int u = 0; u < kDepth; ++u) {
                const int j = base + u * kBlock + (int)threadIdx.x;
                if (j < n16) dst[j] = v[u];
            }
        }
        __syncthreads();
        ltab = reinterpret_cast<const char*>(dst);
        ltv.x0 = vg(lt_arg.x0); ltv.y0 = vg(lt_arg.y0); ltv.inv = vg(lt_arg.inv);
        ltv.nx = vg(lt_arg.nx); ltv.nx_last = vg(lt_arg.nx_last); ltv.ny_last = vg(lt_arg.ny_last);
        ltv.off_l1 = vg(lt_arg.off_l1); ltv.off_sub = vg(lt_arg.off_sub); ltv.off_line = vg(lt_arg.off_line); ltv.off_hts = vg(lt_arg.off_hts);
        ltv.off_resid = vg(lt_arg.off_resid);
    }
    if (!ONE) settle_state(ls, es);
    for (int step = 0; step < n_steps; ++step) {
#if ATC_TRACE
        unsigned long long* trow = trace ? trace + ((size_t)(blockIdx.x * (kBlock / 64) + (tid >> 6)) * n_steps + step) * 8 : nullptr;
        if (lane == 0 && trow) trow[0] = step ? __builtin_amdgcn_s_memtime() : t_launch;
#endif
        const size_t sBN = (size_t)step * BN, sB = (size_t)step * (uint32_t)B;  // uniform (scalar) per-step bases
        // Multi-step launches, history: before the by-value arguments were re-read from the kernarg segment (below), everything
        // invariant across steps (lane ids, the address arithmetic on them, the sector base) had to be re-derived from an opaque
        // zero inside the body, or LICM kept it alive around the loop and the 80-VGPR form spilled 88 B per lane.  With the
        // re-reads the plain form is the faster one (12-20 B of scratch in some widths notwithstanding: 13.70 vs 13.80 us per
        // step, 8 192 x 16 3.98 vs 4.05, profiles/r02_experiments.txt); the knob remains for A/B builds.
        LaneIds dl = d;
        const float* Kl = K;
        const float* gl = grid;
        atc_params_t pl = p;
        atc_out_t outl = out;
        int32_t* stats_l = st.stats;
        int zk = 0;   // this step's opaque zero: kernarg re-reads that depend on it cannot be hoisted out of the step loop
        if (!ONE) {   // (also makes the mode word's flag tests scalar compares inside the step, not
            zk = opaque_zero();   // 64-bit lane masks kept — and spilled — across the loop)
            pl.mode += (uint32_t)zk;
        }
        StepOut so = {outl.obs + sBN * ATC_OBS_DIM, outl.flags + sBN, outl.reward + sB, outl.done + sB,
                      FULL && outl.raw_obs ? outl.raw_obs + sBN * ATC_OBS_DIM : nullptr,
                      FULL && outl.ac_reward ? outl.ac_reward + sBN : nullptr,
                      FULL && outl.min_sep ? outl.min_sep + sB : nullptr,
                      FULL && outl.term_obs ? outl.term_obs + sBN * ATC_OBS_DIM : nullptr,
                      FULL && outl.packet ? outl.packet + sB * (ATC_PKT_CHUNKS * 4) : nullptr
#if ATC_TRACE
                      , trow
#endif
        };
        // Carried across the steps of a multi-step launch: the DECODED targets and the refused-target mask of a held action block
        // (r05: 65 536 x 16 fused 11.8-12.0 -> 11.6-11.8 us) and "every lane's aircraft is under control" (re-established after
        // steps that can change a mask: 11.37 vs 11.46 us).
        const QRates qr = qr_next;
        const QScan qs = QGET(s);   // (requested here, consumed after the kinematics)
        if (!ONE && ATC_RARE(step == 0)) act = *at<Float3>(act_t, times12(dl.i));
        if (ONE || step == 0) tg = decode_targets(qr, act);
        if (ONE && !la_live) {   // held block: the record equals the accepted targets (components that are refused are not compared)
            ls.la_v = tg.v;
            ls.la_h = altitude_target(qr, tg.ah);
            ls.la_p = tg.p;
        }
        // multi-step launches know structurally which steps repeat an action block
        const bool repeated = ONE ? (same_actions && __builtin_amdgcn_ballot_w64(la_live) == 0ull)
                                  : (!block_start && __builtin_amdgcn_ballot_w64(es.t == 0) == 0ull);
        // ... and whether every lane's aircraft is under control: re-established after the steps in which a mask can change
        if (!ONE && ATC_RARE(mask_dirty)) {
            // (and no lane's heading or last heading target is WIDE: include/atc_step.h ABI 19 — such lanes take the general form)
            all_active = (__builtin_amdgcn_ballot_w64(!(dl.lane_valid && ((dl.k < 32 ? ((uint32_t)es.amask >> dl.k) : ((uint32_t)(es.amask >> 32) >> (dl.k - 32))) & 1u))) |
                          __builtin_amdgcn_ballot_w64(max(ls.a.phi, ls.la_p) == INT32_MAX) | __builtin_amdgcn_ballot_w64(min(ls.a.phi, ls.la_p) == INT32_MIN)) == 0ull;
            mask_dirty = false;
        }
        ATC_STAMP_TOP(trow, 1);
        const Mid m = step_part_a<ONE, LAT, LDSG>(gl, qr, QGET(k), QGET(g), dl, tg.v, altitude_target(qr, tg.ah), tg.p, act.c, ls, es, repeated, !ONE && all_active,
                                             st.phi_wide, zk, refused_blk, refused_known ATC_TRACE_PASS(trow), ltab, &ltv);
        refused_known = true;
        ATC_STAMP(1);
        Float3 nxt = act;
        const float* act_next = nullptr;   // the next block is fetched during the last step of the current one
        block_start = false;
        if (!ONE && ATC_RARE(--left == 0)) {   // (the block length is fetched again here, at block ends, not kept — or re-fetched — every step)
            left = kernarg_reread<int>(offsetof(StepArgs, hold), zk);
            block_start = true;
            refused_known = false;
            act_t += (size_t)BN * 3;
            if (step + 1 < n_steps) act_next = act_t;
        }
        const bool quiet = step_part_b<W, FULL, ONE, LAT, LDSG>(Kl, gl, pl, q, qs, zk, N, dl, m, ls, es, so, stats_l, st.phi_wide, pos, obs_stage, act_next, nxt, qr_next, scan_skip, scan_mask, ltab, &ltv);
        if (ATC_RARE(!quiet)) mask_dirty = true;
        if (act_next) tg = decode_targets(QGET(r), nxt);
        act = nxt;
        ATC_STAMP(6);
        ATC_STAMP_TOP(trow, 6);
        ATC_STAMP_END(trow, 6);
    }
    // ---- write back persistent state -----------------------------------------------------------------------------------
    atc_state_t st_end = st;
    // (single-step launches also fetch the state pointers again for the final stores instead of carrying ten scalar registers
    // through the body: they were spilled to vector-register lanes)
    if (ONE || loop_rereads_state(W)) st_end = kernarg_reread<atc_state_t>(offsetof(StepArgs, st), opaque_zero());
    store_lane_state(st_end, d, ls, la_live);
    store_env_state<W>(st_end, d, es, hi0);
    if (ATC_KARG_PREFETCH(W, ONE)) asm volatile("" ::"s"(karg_touch));   // (keeps the touches alive; nothing waits for them before here)
    if (ATC_FILL_PREFETCH(W, FULL, ONE, ALLV)) asm volatile("" ::"v"(pf_ac), "v"(pf_alt));   // (the prefetched words: discarded here)
#if ATC_TRACE
    if (lane == 0 && trace) trace[((size_t)(blockIdx.x * (kBlock / 64) + (tid >> 6)) * n_steps + (n_steps - 1)) * 8 + 7] = __builtin_amdgcn_s_memtime();
#endif
}
// StepArgs is k_step's list: every member that an offsetof(StepArgs, ...) names, and the last one — a parameter added to one of the two
// alone does not compile.  (The layout does not depend on the template arguments: one instance stands for all.)
typedef KernArgs<decltype(k_step<1, false, true, true>)> StepKernArgs;
static_assert(kernargs_hold_like_step<decltype(k_step<1, false, true, true>)>() && StepKernArgs::of<LdsTab>() == offsetof(StepArgs, lt) &&
                  StepKernArgs::last() == offsetof(StepArgs, pf_stride),
              "StepArgs must list k_step's parameters in order: the step re-reads them by StepArgs offsets");

// ---------------------------------------------------------------------------------------------------------------
// Frame skip (include/atc_step.h: atc_step_skip): up to K steps with ONE held action block in one launch, ONE set of outputs.
// Per env: step until the step reports done or K steps are taken; outputs = the last executed step's observation, the float32 sums
// of the executed steps' rewards in step order, the OR of their flag words, the minimum of their separations, done, n.
//   State is loaded once and kept in registers like in the multi-step k_step; every step runs step_part_a / step_part_b<SKIP> — the
//   arithmetic of atc_step with the per-step stores taken out — and four accumulators are carried across the loop.  An env STORES
//   its outputs and its state at the end of its last executed step (`fin`), inside the loop: a wavefront whose envs all run K steps
//   — almost every one — stores once, behind the last step, with the observation on the transposed 16-byte path; a wavefront in
//   which an env ends early stores that env's rows then and the others' later.  Nothing of the kept observation lives across a step.
//   A STOPPED env has no further effect, because from the step after its last
//     * its lanes run with env_valid = lane_valid = false in that step's LaneIds: `done` is `d.env_valid && ...`, so no second
//       reset and no write of the per-episode record; the side records of WIDE headings and the terminal observation are
//       written under lane_valid only;
//     * its bit in `live` is cleared, and outputs and state are stored under `fin`, a subset of `live`: what its lanes go on
//       computing on their stale registers is never stored, added to anything that is, or read by another env (group reductions
//       and the separation scan stay inside the W lanes of an env; wave-uniform shortcuts — plain, quiet, all_active — only choose
//       between forms that evaluate the same expressions per lane).
//   The loop ends when no env of the wavefront is live.  Steps after the first repeat the block's actions on envs that were not
//   reset in between (a reset env is stopped): `repeated`, the structural form of ATC_M_ACTIONS_HELD.
//   The argument list is k_step's up to `q` (StepArgs): step_part_a / step_part_b re-read state pointers and derived constants from
//   the kernarg segment by those offsets (the static_assert behind the kernel holds its list to them).  The separation-scan horizon is left off (full scan in every step).
//   FULL: an optional output (raw_obs, ac_reward, min_sep, term_obs) is requested — as in k_step the fast form compiles them out
//   (no raw observation in registers, the conflict-only scan); which of them is present is a run-time null test in the full form.
//   Registers, launch bound: DESIGN.md, frame skip.
// ---------------------------------------------------------------------------------------------------------------
// wavefronts per SIMD k_skip is register-budgeted for (<= 96 VGPRs).  Measured against 4 (no spills, slower) and against 6 for the
// fast form of 16-aircraft envs (k_step's rule for its loop forms: no faster here): DESIGN.md, frame skip.  -DATC_SKIP_WAVES=n: A/B builds.
#ifndef ATC_SKIP_WAVES
#define ATC_SKIP_WAVES 5
#endif
template <int W, bool FULL>
__global__ void __launch_bounds__(kBlock, ATC_SKIP_WAVES)
k_skip(const float* __restrict__ blob, int off_grid, int B, int N, int K_steps, int pad, atc_state_t st,
       const float* __restrict__ actions, atc_out_t out, atc_params_t p, StepDerived q, uint8_t* n_steps) {
    constexpr bool ONE = false, LAT = false;   // (QGET: the multi-step form — kernarg re-reads inside the step)
    extern __shared__ __attribute__((aligned(16))) float smem[];
    float4* pos = reinterpret_cast<float4*>(smem);                    // [2 kBlock] pair-scan staging (W >= 32)
    float* obs_stage = smem + (W >= 32 ? 2 * kBlock * 4 : 0);  // [4 waves][64 x 10] obs transpose
    const float* __restrict__ K = blob;
    const float* __restrict__ grid = off_grid ? blob + off_grid : nullptr;
    const LaneIds d = make_ids<W, false>(blockIdx.x * kBlock, B, N);

    const int4 e0 = *at<int4>(st.env, (uint32_t)d.e * (ATC_ENV_WORDS * 4u));
    const uint32_t hi0 = (W == 64) ? *at<uint32_t>(st.stats, (uint32_t)d.e * (ATC_STAT_WORDS * 4u) + ATC_STAT_MASK_HI * 4u) : 0u;
    EnvState es = {e0.x, e0.y, __int_as_float(e0.z), (uint64_t)(uint32_t)e0.w | ((uint64_t)hi0 << 32)};
    const int4 ps = *at<int4>(st.ac, d.i * 16u);
    const double h0 = *at<double>(st.alt, d.i * 8u);
    const Float3 act = *at<Float3>(actions, times12(d.i));   // the block's action: one 12-byte load per lane
    const int4 la0 = *at<int4>(st.last_act, d.i * 16u);      // (the block's first step carries a fresh decision: the record is live)
    LaneState ls = {{ps.x, ps.y, h0, ps.z, (uint32_t)ps.w}, (uint32_t)la0.x, __hiloint2double(la0.w, la0.z), la0.y, false};

    Targets tg = {0u, 0.0f, 0};
    uint64_t refused_blk = 0ull;
    bool refused_known = false;
    bool all_active = false, mask_dirty = true;
    QRates qr_next = kernarg_reread<QRates>(offsetof(StepArgs, q) + offsetof(StepDerived, r), opaque_zero());
    settle_state(ls, es);
    // accumulated over the executed steps, in step order: plain float32 additions (the library is built with -ffp-contract=off)
    float sum_r = 0.0f, sum_env = 0.0f, min_d2 = 1e30f;
    uint32_t or_fl = 0u;
    uint64_t live = __builtin_amdgcn_ballot_w64(d.env_valid);   // lanes of envs that have not taken their last step (uniform per env)
    for (int step = 0; live != 0ull; ++step) {
        LaneIds dl = d;
        const bool lane_live = ((live >> d.lane) & 1ull) != 0ull;
        dl.env_valid = lane_live;
        dl.lane_valid = d.lane_valid && lane_live;
        atc_params_t pl = p;
        const int zk = opaque_zero();   // this step's opaque zero (see k_step)
        pl.mode += (uint32_t)zk;
        const atc_out_t outl = out;
        const StepOut so = {outl.obs, outl.flags, outl.reward, outl.done, FULL ? outl.raw_obs : nullptr, FULL ? outl.ac_reward : nullptr,
                            FULL ? outl.min_sep : nullptr, FULL ? outl.term_obs : nullptr, nullptr};
        const QRates qr = qr_next;
        const QScan qs = QGET(s);
        if (ATC_RARE(step == 0)) tg = decode_targets(qr, act);
        const bool repeated = step != 0;
        if (ATC_RARE(mask_dirty)) {
            all_active = (__builtin_amdgcn_ballot_w64(!(dl.lane_valid && ((dl.k < 32 ? ((uint32_t)es.amask >> dl.k) : ((uint32_t)(es.amask >> 32) >> (dl.k - 32))) & 1u))) |
                          __builtin_amdgcn_ballot_w64(max(ls.a.phi, ls.la_p) == INT32_MAX) | __builtin_amdgcn_ballot_w64(min(ls.a.phi, ls.la_p) == INT32_MIN)) == 0ull;
            mask_dirty = false;
        }
        const Mid m = step_part_a<false, false>(grid, qr, QGET(k), QGET(g), dl, tg.v, altitude_target(qr, tg.ah), tg.p, act.c, ls, es, repeated, all_active,
                                                st.phi_wide, zk, refused_blk, refused_known ATC_TRACE_PASS(nullptr));
        refused_known = true;
        StepVals sv;
        Float3 nxt = act;
        int scan_skip = 0;
        uint32_t scan_mask = 0u;
        const bool quiet = step_part_b<W, FULL, false, false, false, true>(K, grid, pl, q, qs, zk, N, dl, m, ls, es, so, st.stats, st.phi_wide, pos, obs_stage,
                                                                            nullptr, nxt, qr_next, scan_skip, scan_mask, nullptr, nullptr, &sv);
        if (ATC_RARE(!quiet)) mask_dirty = true;
        // acc = r1; acc = acc + r2; ...  (the first step assigns: 0 + r would turn a -0 into +0)
        sum_r = repeated ? sum_r + sv.r : sv.r;
        sum_env = repeated ? sum_env + sv.env_r : sv.env_r;
        or_fl |= sv.fl;
        if (FULL) min_d2 = fminf(min_d2, sv.min_d2);   // (sqrt is monotonic: the minimum of the roots is the root of the minimum)
        // envs that have just taken their last step: done, or the block's K-th
        const uint64_t fin = (step + 1 >= K_steps) ? live : (live & __builtin_amdgcn_ballot_w64(sv.done));
        if (fin != 0ull) {
            LaneIds df = d;
            const bool mine = ((fin >> d.lane) & 1ull) != 0ull;
            df.env_valid = mine;
            df.lane_valid = d.lane_valid && mine;
            df.wave_full = d.wave_full && fin == ~0ull;
            const int zs = opaque_zero();
            const atc_state_t st_end = kernarg_reread<atc_state_t>(offsetof(StepArgs, st), zs);
            const atc_out_t o_end = kernarg_reread<atc_out_t>(offsetof(StepArgs, out), zs);
            store_obs_rows(o_end.obs, df, sv.o, obs_stage);
            if (df.lane_valid) {
                if (FULL && o_end.raw_obs) store_obs(at<float>(o_end.raw_obs, times40(d.i)), sv.zraw);
                stream_store(at<uint16_t>(o_end.flags, d.i * 2u), (uint16_t)or_fl);
                if (FULL && o_end.ac_reward) *at<float>(o_end.ac_reward, d.i * 4u) = sum_r;
            }
            if (mine && d.k == 0) {
                *at<float>(o_end.reward, (uint32_t)d.e * 4u) = sum_env;
                *at<uint8_t>(o_end.done, (uint32_t)d.e) = sv.done ? 1 : 0;
                if (FULL && o_end.min_sep) *at<float>(o_end.min_sep, (uint32_t)d.e * 4u) = (min_d2 >= 1e30f) ? 1e30f : sqrtf(min_d2);
                if (n_steps) *at<uint8_t>(n_steps, (uint32_t)d.e) = (uint8_t)(step + 1);
            }
            store_lane_state(st_end, df, ls, true);
            store_env_state<W>(st_end, df, es, hi0);
            live &= ~fin;
        }
    }
}
static_assert(kernargs_like_step<decltype(k_skip<1, false>)>(), ATC_KERNARGS_REFUSAL);

// ---------------------------------------------------------------------------------------------------------------
// Persistent step server of ONE env x ONE aircraft (the drop-in AtcGym, atc_gym.py:128-192; include/atc_step.h: atc_serve_*).
// One resident wavefront keeps the env's state in registers and polls a mailbox in pinned mapped host memory: the host writes
// {action, sequence number} with ONE 16-byte store, the wavefront runs the single-step body (the same step_part_a / step_part_b
// as k_step<1, FULL, ONE>) and answers with the self-validating result packet (atc_out_t.packet).  No launch, no kernel-argument
// upload and no state round trip per step: what is left is two crossings of the host link and the step's own dependent chain.
// It LEAVES — state written back, mailbox status updated — on the quit command or after `lease_ticks` of s_memrealtime (100 MHz)
// without a command: a host that died or went to train for a minute never leaves a wavefront spinning.
// ---------------------------------------------------------------------------------------------------------------
enum { ATC_MB_CMD = 0, ATC_MB_SEQ = 3, ATC_MB_STATE = 4, ATC_MB_LAST = 5, ATC_MB_WORDS = 16 };
enum { ATC_SERVE_IDLE = 0, ATC_SERVE_RUNNING = 1, ATC_SERVE_LEFT_LEASE = 2, ATC_SERVE_LEFT_QUIT = 3 };
#define ATC_SERVE_QUIT 0xffffffffu
__device__ __forceinline__ uint32_t mb_load(const uint32_t* w) {
    return __hip_atomic_load(w, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
}
__global__ void __launch_bounds__(64, 1)
k_serve(const float* __restrict__ blob, int off_grid, atc_state_t st, atc_out_t out, atc_params_t p, StepDerived q_arg,
        uint32_t* mailbox, uint32_t last, unsigned long long lease_ticks) {
    // (one wavefront alone on its SIMD: the uniform terms live in vector registers like in the latency-bound instantiation — as
    // named scalar arguments kept across the serving loop, 151 of them were spilled to vector-register lanes)
    const StepDerived q = to_vector_registers(q_arg);
    extern __shared__ __attribute__((aligned(16))) float smem[];
    const float* __restrict__ K = blob;
    const float* __restrict__ grid = off_grid ? blob + off_grid : nullptr;
    const LaneIds d = make_ids<1, false>(0u, 1, 1);   // lane 0 is the aircraft; the other lanes compute on copies and store nothing
    const int4 e0 = *at<int4>(st.env, 0u);
    EnvState es = {e0.x, e0.y, __int_as_float(e0.z), (uint64_t)(uint32_t)e0.w};
    const int4 ps = *at<int4>(st.ac, 0u);
    const double h0 = *at<double>(st.alt, 0u);
    const int4 la0 = *at<int4>(st.last_act, 0u);
    LaneState ls = {{ps.x, ps.y, h0, ps.z, (uint32_t)ps.w}, (uint32_t)la0.x, __hiloint2double(la0.w, la0.z), la0.y, false};
    const StepOut so = {out.obs, out.flags, out.reward, out.done, out.raw_obs, out.ac_reward, out.min_sep, out.term_obs, out.packet};
    if (threadIdx.x == 0) __hip_atomic_store(mailbox + ATC_MB_STATE, (uint32_t)ATC_SERVE_RUNNING, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
    unsigned long long t_cmd = __builtin_amdgcn_s_memrealtime();
    uint32_t left_as = ATC_SERVE_LEFT_LEASE;
    for (;;) {
        // (every lane reads the same word: one request; made wave-uniform for the control flow)
        const uint32_t seq = (uint32_t)__builtin_amdgcn_readfirstlane((int)__hip_atomic_load(mailbox + ATC_MB_SEQ, __ATOMIC_ACQUIRE, __HIP_MEMORY_SCOPE_SYSTEM));
        if (seq == ATC_SERVE_QUIT) {
            left_as = ATC_SERVE_LEFT_QUIT;
            break;
        }
        if (seq != last + 1u) {
            if (__builtin_amdgcn_s_memrealtime() - t_cmd > lease_ticks) break;
            continue;
        }
        // the action travelled in the same 16-byte host store as its sequence number
        const Float3 act = {__uint_as_float(mb_load(mailbox + ATC_MB_CMD)), __uint_as_float(mb_load(mailbox + ATC_MB_CMD + 1)),
                            __uint_as_float(mb_load(mailbox + ATC_MB_CMD + 2))};
        last = seq;
        atc_params_t pl = p;
        pl.reserved0 = seq;   // the packet's tag (step_part_b)
        const Targets tg = decode_targets(q.r, act);
        uint64_t refused = 0ull;
        const Mid m = step_part_a<true, true>(grid, q.r, q.k, q.g, d, tg.v, altitude_target(q.r, tg.ah), tg.p, act.c, ls, es, false, false,
                                               st.phi_wide, 0, refused, false ATC_TRACE_PASS(nullptr));
        Float3 nxt = act;
        QRates qn = q.r;
        int scan_skip = 0;
        uint32_t scan_mask = 0u;
        step_part_b<1, true, true, true>(K, grid, pl, q, q.s, 0, 1, d, m, ls, es, so, st.stats, st.phi_wide, nullptr, smem, nullptr, nxt, qn,
                                          scan_skip, scan_mask);
        t_cmd = __builtin_amdgcn_s_memrealtime();
    }
    store_lane_state(st, d, ls, true);
    store_env_state<1>(st, d, es, 0u);
    __threadfence_system();
    if (threadIdx.x == 0) {
        __hip_atomic_store(mailbox + ATC_MB_LAST, last, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
        __hip_atomic_store(mailbox + ATC_MB_STATE, left_as, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
    }
}

#include "atc_aux_kernels.inc"   // k_reset, k_observe, k_reset_env, k_query_*
#include "atc_traffic.inc"       // k_traffic (atc_observe_traffic)
#include "atc_lookahead.inc"     // k_lookahead (atc_lookahead)
#include "atc_plan.inc"          // k_plan (atc_lookahead_plan)
#include "atc_plan_sampled.inc"  // k_plan_sampled (atc_lookahead_plan_sampled), k_plan_draw (atc_plan_draw)
#include "atc_plan_refit.inc"    // k_plan_refit (atc_plan_refit)
#include "atc_plan_score.inc"    // k_plan_score (atc_plan_score)
#include "atc_branch.inc"        // k_branch (atc_branch), k_select (atc_state_select)
#include "atc_policy.inc"        // k_rollout_policy (atc_rollout_policy), k_rollout_policy_traffic (atc_rollout_policy_traffic), k_rollout_policy_ends (atc_rollout_policy_ends)
#include "atc_lookahead_policy.inc"   // k_lookahead_policy (atc_lookahead_policy): k_plan_sampled's loop with policy_decide where it draws
#include "atc_gae.inc"           // k_gae (atc_gae), k_gae_boot (atc_gae_boot)
#include "atc_ppo_grad.inc"      // k_ppo_grad, k_ppo_grad_reduce (atc_ppo_policy_grad)
#include "atc_value.inc"         // k_value_forward (atc_value_forward), k_ppo_value_grad, k_ppo_value_grad_reduce (atc_ppo_value_grad)
#include "atc_policy_forward.inc"  // k_policy_forward (atc_policy_forward)
#include "atc_ppo_update.inc"    // k_adv_moments, k_adv_apply (atc_adv_normalise), k_adam_step (atc_adam_step)

// ---------------------------------------------------------------------------------------------------------------
// host side of the C-ABI
// ---------------------------------------------------------------------------------------------------------------
#include <initializer_list>
#include <utility>
static int grid_for(const atc_scenario* s, long long threads) {
    long long blocks = (threads + kBlock - 1) / kBlock;
    const long long cap = (long long)s->n_cu * ATC_GRID_CAP;
    if (blocks > cap) blocks = cap;
    if (blocks < 1) blocks = 1;
    return (int)blocks;
}
// the step kernels (k_step, k_skip): one workgroup per 256 slots of W per env, no grid-stride loop
static int step_grid(int B, int W) { return (int)(((long long)B * W + kBlock - 1) / kBlock); }
// ... and the kernels over the flat B*N aircraft of a plan (k_plan_draw, k_plan_refit): the same tiles of 256, no padding to W
static unsigned flat_tiles(int B, int N) { return (unsigned)step_grid(B, N); }
static size_t lds_bytes(const atc_scenario*, bool pair_scan, bool step_kernel = false) {
    size_t w = 0;  // the sector is not staged: LDS only holds the obs transpose stage and the pair-scan staging
    if (step_kernel) w += (size_t)(kBlock / 64) * 64 * ATC_OBS_DIM;
    if (pair_scan) w += (size_t)2 * kBlock * 4;
    return w * sizeof(float);
}

// the launch records (include/atc_step.h: the atc_*_launch_counts getters): launches made by the calling thread, every record's
// counters in one table — plain thread-local counters that nothing in the library reads back.  REC_STEP has a slot for each k_step
// instantiation and one for k_serve starts; a record of 7 slots counts by lane-group width (slot = log2(W)); a record of one slot
// counts its entry point's launches; REC_POLICY_TRAFFIC and REC_POLICY_TERM count by width and list length (slot = 3 log2(W) + log2(K)), REC_POLICY_ENDS
// and REC_POLICY_EVAL likewise with K = 0 in front (slot = 4 log2(W) + {0, 1, 2, 3}); REC_PPO_GRAD, REC_VALUE_FORWARD, REC_PPO_VALUE_GRAD and REC_POLICY_FORWARD count calls by K
// (slot = {0, 1, 2, 3}); REC_ADV_NORMALISE counts calls in one slot and REC_ADAM_STEP by the number of tensors (slot = n_tensors - 1).  A call
// moves its own record only.
enum Record { REC_STEP, REC_SKIP, REC_TRAFFIC, REC_LOOKAHEAD, REC_PLAN, REC_PLAN_SAMPLED, REC_PLAN_DRAW, REC_PLAN_REFIT, REC_PLAN_SCORE, REC_BRANCH, REC_SELECT, REC_POLICY, REC_POLICY_TRAFFIC, REC_GAE, REC_POLICY_ENDS, REC_GAE_BOOT, REC_PPO_GRAD, REC_VALUE_FORWARD, REC_PPO_VALUE_GRAD, REC_POLICY_EVAL, REC_ADV_NORMALISE, REC_ADAM_STEP, REC_POLICY_FORWARD, REC_LOOKAHEAD_POLICY, REC_POLICY_TERM, REC_COUNT };
constexpr int kRecordSlots[REC_COUNT] = {ATC_LAUNCH_SLOTS, ATC_SKIP_LAUNCH_SLOTS, ATC_TRAFFIC_LAUNCH_SLOTS, ATC_LOOKAHEAD_LAUNCH_SLOTS, ATC_PLAN_LAUNCH_SLOTS,
                                         ATC_PLAN_SAMPLED_LAUNCH_SLOTS, ATC_PLAN_DRAW_LAUNCH_SLOTS, ATC_PLAN_REFIT_LAUNCH_SLOTS, ATC_PLAN_SCORE_LAUNCH_SLOTS,
                                         ATC_BRANCH_LAUNCH_SLOTS, ATC_SELECT_LAUNCH_SLOTS, ATC_ROLLOUT_POLICY_LAUNCH_SLOTS,
                                         ATC_ROLLOUT_POLICY_TRAFFIC_LAUNCH_SLOTS, ATC_GAE_LAUNCH_SLOTS, ATC_ROLLOUT_POLICY_ENDS_LAUNCH_SLOTS,
                                         ATC_GAE_BOOT_LAUNCH_SLOTS, ATC_PPO_GRAD_LAUNCH_SLOTS, ATC_VALUE_FORWARD_LAUNCH_SLOTS,
                                         ATC_PPO_VALUE_GRAD_LAUNCH_SLOTS, ATC_POLICY_EVAL_LAUNCH_SLOTS, ATC_ADV_NORMALISE_LAUNCH_SLOTS,
                                         ATC_ADAM_STEP_LAUNCH_SLOTS, ATC_POLICY_FORWARD_LAUNCH_SLOTS, ATC_LOOKAHEAD_POLICY_LAUNCH_SLOTS,
                                         ATC_ROLLOUT_POLICY_TERM_LAUNCH_SLOTS};
constexpr int record_offset(int id) {
    int o = 0;
    for (int i = 0; i < id; ++i) o += kRecordSlots[i];
    return o;
}
static thread_local uint64_t t_records[record_offset(REC_COUNT)] = {0};
static uint64_t* record(int id) { return t_records + record_offset(id); }

// Fill-phase prefetch of the fast single-step launches (k_step): `stride` = the workgroups the device holds at once = the first
// round of the launch, from the runtime's occupancy for the instantiation (asked once per thread, instantiation and device) and the
// device's CU count, rounded DOWN to a multiple of 8: workgroups are dealt round-robin to the 8 XCDs, so workgroup j + stride runs
// on the XCD whose L2 workgroup j prefetched into.  0 (off) for a grid that fits the first round, and with ATC_NO_FILL_PREFETCH set
// in the environment (developer knob, read once per process: the A/B run and tests/test_fill_prefetch.py).
static bool fill_prefetch_enabled() {
    static const bool on = [] { const char* e = getenv("ATC_NO_FILL_PREFETCH"); return !(e && *e && strcmp(e, "0") != 0); }();
    return on;
}
// Residency cap of the same launches (profiles/step_resident_ab.txt): the kernel's registers let a CU hold 7
// workgroups, by estimate more than the memory system needs in flight, at about half a workgroup lifetime lost at either end.  A cap
// of k workgroups per CU is made with LDS the kernel never touches: the launch asks for so much dynamic LDS — padding BEHIND the obs
// transpose stage, the only LDS these forms use, so no offset in the kernel moves — that the CU's LDS holds exactly k workgroups
// (the largest multiple of the allocation granule that is <= cu_lds / k).  The runtime's occupancy for the padded size must confirm k;
// if it does not, the launch stays unpadded.  Only a grid of more than k workgroups per CU is padded: a smaller one fits either way.
//   kStepResident<W>: the shipped cap per lane-group width (0 = none), chosen by measurement — and the measurement says none: 6 is
//   level with the registers' 7, 5 costs 3 % and 4 costs 9 % at 65 536 x 16, the same order at W = 8 and at four times the envs (the
//   front and the tail of the launch do get shorter, the streaming body loses more).  ATC_STEP_RESIDENT=<k> in the
//   environment (developer knob, read once per process: the sweep and tests/test_step_resident.py) forces k = 1..8 for every width;
//   0, or a k at or above what the registers allow, means no padding.
template <int W>
constexpr int kStepResident = 0;
constexpr int kLdsGranule = 1280;   // gfx950 allocates LDS in granules of 320 dwords
static int step_resident_knob() {   // -1: unset
    static const int k = [] {
        const char* e = getenv("ATC_STEP_RESIDENT");
        if (!e || !*e) return -1;
        const int v = atoi(e);
        return v < 0 ? 0 : v > 8 ? 8 : v;
    }();
    return k;
}
struct StepResidency {
    int per_cu;   // workgroups a CU holds at once in a launch of more than per_cu * n_cu workgroups
    size_t pad;   // dynamic LDS bytes such a launch requests beyond lds_bytes() (0: residency is what the registers allow)
};
template <int W>
static int step_residency(const atc_scenario* s, StepResidency* out) {   // (asked once per thread, instantiation and device)
    static thread_local int cached_for = -1;
    static thread_local StepResidency cached = {0, 0};
    if (cached_for != s->device) {
        const void* fn = reinterpret_cast<const void*>(&k_step<W, false, true, true>);
        const size_t base = lds_bytes(s, W >= 32, true);
        int free_wgs = 0;
        HIP_TRY(hipOccupancyMaxActiveBlocksPerMultiprocessor(&free_wgs, fn, kBlock, base));
        StepResidency r = {free_wgs, 0};
        const int cap = step_resident_knob() >= 0 ? step_resident_knob() : kStepResident<W>;
        if (cap >= 1 && cap < free_wgs) {
            const size_t want = (size_t)(s->cu_lds / cap) / kLdsGranule * kLdsGranule;
            int capped = 0;
            if (want > base && want <= (size_t)s->max_lds &&   // (a cap of 3 or lower needs more than 48 KB: the launch raises the attribute)
                (want <= 48 * 1024 || hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, s->max_lds) == hipSuccess) &&
                hipOccupancyMaxActiveBlocksPerMultiprocessor(&capped, fn, kBlock, want) == hipSuccess && capped == cap)
                r = StepResidency{cap, want - base};
            (void)hipGetLastError();
        }
        cached = r;
        cached_for = s->device;
    }
    *out = cached;
    return ATC_OK;
}
template <int W>
static int fill_prefetch_resident(const atc_scenario* s, int* resident) {
    StepResidency r;
    if (const int rc = step_residency<W>(s, &r)) return rc;
    *resident = (r.per_cu * s->n_cu) & ~7;
    return ATC_OK;
}

template <int W, bool FULL, bool ONE, bool ALLV, bool LAT = false, bool LDSG = false>
static int launch_step2(const atc_scenario* s, int B, int N, int T, int hold, const atc_state_t* st, const float* actions,
                        const atc_out_t* out, const atc_params_t* p, hipStream_t stream) {
    size_t lds = lds_bytes(s, W >= 32, true) + (LDSG ? s->lds_tab_bytes : 0);
    const int grid = step_grid(B, W);
    int pf_stride = 0;
    if constexpr (ATC_FILL_PREFETCH(W, FULL, ONE, ALLV)) {
        StepResidency r;
        if (const int rc = step_residency<W>(s, &r)) return rc;
        if ((long long)grid > (long long)r.per_cu * s->n_cu) lds += r.pad;   // (the residency cap: see step_residency)
        if (fill_prefetch_enabled()) {
            pf_stride = (r.per_cu * s->n_cu) & ~7;
            if (grid <= pf_stride) pf_stride = 0;
        }
    }
    if (lds > 48 * 1024) {   // (once per device and instantiation: the attribute sticks)
        static thread_local int raised_for = -1;
        if (raised_for != s->device) {
            HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void*>(&k_step<W, FULL, ONE, ALLV, LAT, LDSG>),
                                        hipFuncAttributeMaxDynamicSharedMemorySize, s->max_lds));
            raised_for = s->device;
        }
    }
    LdsTab lt = s->lt;
    if (!LDSG) lt.src = nullptr;
    hipLaunchKernelGGL((k_step<W, FULL, ONE, ALLV, LAT, LDSG>), dim3(grid), dim3(kBlock), lds, stream, s->d_blob, s->off_grid, B, N, T, hold, *st, actions, *out, *p, derive(*p, s, scan_horizon<W, FULL, ONE>()), inline_action(), lt, pf_stride);
    HIP_TRY(hipGetLastError());
    constexpr int form = LDSG ? ATC_LF_LDSG : LAT ? ATC_LF_LAT : FULL ? (ONE ? ATC_LF_FULL_ONE : ATC_LF_FULL_MULTI)
                         : ONE ? (ALLV ? ATC_LF_ALLV_ONE : ATC_LF_GEN_ONE) : (ALLV ? ATC_LF_ALLV_MULTI : ATC_LF_GEN_MULTI);
    ++record(REC_STEP)[__builtin_ctz(W) * ATC_LF_FORMS + form];
    return ATC_OK;
}
template <int W>
static int launch_step(const atc_scenario* s, int B, int N, int T, int hold, const atc_state_t* st, const float* actions,
                       const atc_out_t* out, const atc_params_t* p, hipStream_t stream) {
    const bool full = out->raw_obs || out->ac_reward || out->min_sep || out->term_obs || out->packet;
    // every slot of the launch is an aircraft: the fast variant then runs its all-valid instantiation (make_ids)
    const bool allv = !full && N == W && ((long long)B * W) % kBlock == 0;
    // Multi-step launches keep the state in registers across the steps; the run-time step loop costs the kernel its
    // occupancy (4 wavefronts per SIMD against 5-7 for the straight-line single step) but issuing T single-step launches
    // instead is slower at every size (65 536 x 16, T = 20, [T, ...] outputs: 35.0 vs 27.1 us per step).
    if (T > 1) {
        if (full) return launch_step2<W, true, false, false>(s, B, N, T, hold, st, actions, out, p, stream);
        // at most ATC_LAT_WAVES wavefronts per SIMD: the latency-bound instantiation (uniform terms in vector registers)
        const bool lat = allv && ((long long)B * W + 63) / 64 <= (long long)ATC_LAT_WAVES * 4 * s->n_cu;
        // ... of one-aircraft envs, at most one workgroup per CU, a lookup table attached: the table lives in LDS for the launch
        if constexpr (W == 1) {
            if (lat && s->lt.src && (long long)B <= (long long)kBlock * s->n_cu && s->off_grid &&
                lds_bytes(s, false, true) + s->lds_tab_bytes <= (size_t)s->max_lds)
                return launch_step2<1, false, false, true, true, true>(s, B, N, T, hold, st, actions, out, p, stream);
        }
        if (lat) return launch_step2<W, false, false, true, true>(s, B, N, T, hold, st, actions, out, p, stream);
        return allv ? launch_step2<W, false, false, true>(s, B, N, T, hold, st, actions, out, p, stream)
                    : launch_step2<W, false, false, false>(s, B, N, T, hold, st, actions, out, p, stream);
    }
    if (full) return launch_step2<W, true, true, false>(s, B, N, 1, 1, st, actions, out, p, stream);
    return allv ? launch_step2<W, false, true, true>(s, B, N, 1, 1, st, actions, out, p, stream)
                : launch_step2<W, false, true, false>(s, B, N, 1, 1, st, actions, out, p, stream);
}

// argument checks shared by every entry point that touches the env state
// the batch shape alone (atc_plan_draw has no state to check): the range of B and N, then the 32-bit byte offsets of one launch over
// B envs (atc_branch: the M*B envs it writes; atc_state_select: either batch), refused in the caller's words
static int check_batch_range(int B, int N) {
    if (B < 1 || N < 1 || N > ATC_MAX_AIRCRAFT) return fail_arg("need B >= 1, 1 <= N <= 64");
    return ATC_OK;
}
static int check_batch_size(unsigned long long B, int N,
                            const char* refusal = "B*N too large for one launch (B*N*40 bytes must stay below 4 GiB): split the batch") {
    if (B * N * ATC_OBS_DIM * 4ull >= (1ull << 32) || B * 64ull >= (1ull << 32)) return fail_arg(refusal);
    return ATC_OK;
}
static bool state_has_null(const atc_state_t* st) {
    return !st->ac || !st->alt || !st->last_act || !st->env || !st->stats || !st->phi_wide;
}
static int check_env_args(const atc_scenario_t* s, int B, int N, const atc_state_t* st, const atc_params_t* p) {
    if (!s || !st || !p) return fail_arg("null pointer");
    if (const int rc = check_batch_range(B, N)) return rc;
    if (state_has_null(st)) return fail_arg("atc_state_t has a null field");
    return check_batch_size(B, N);
}

// the step's time increment against the fixed-point formats of include/atc_step.h: a step's displacement (<= 512 kt) must stay below
// 2^30 position-grid counts and the speed's rate limit below 2^31 speed counts — dt up to 51 s for any sector (the reference uses 1 s)
static int check_dt(const atc_scenario_t* s, const atc_params_t* p) {
    if (!(p->dt > 0.0)) return fail_arg("dt must be > 0");
    if (!(0.1423 * p->dt * (double)s->consts[ATC_C_POS_SCALE] < 1073741824.0) || !((double)kAMax * p->dt < 255.9))
        return fail_arg("dt too large for the fixed-point state formats (see include/atc_step.h)");
    return ATC_OK;
}

static int check_required_outputs(const atc_out_t* out) {
    if (!out->obs || !out->reward || !out->done || !out->flags) return fail_arg("obs/reward/done/flags are required");
    return ATC_OK;
}
// f(std::integral_constant<int, W>) for the lane-group width of N-aircraft envs: W = next_pow2(N)
template <typename F>
static int with_width(int N, F f) {
    if (N == 1) return f(std::integral_constant<int, 1>());
    if (N == 2) return f(std::integral_constant<int, 2>());
    if (N <= 4) return f(std::integral_constant<int, 4>());
    if (N <= 8) return f(std::integral_constant<int, 8>());
    if (N <= 16) return f(std::integral_constant<int, 16>());
    if (N <= 32) return f(std::integral_constant<int, 32>());
    return f(std::integral_constant<int, 64>());
}
// f(std::integral_constant<bool, b>) for a run-time flag
template <typename F>
static int with_flag(bool b, F f) {
    return b ? f(std::true_type()) : f(std::false_type());
}

static int step_common(const atc_scenario_t* s, int B, int N, int T, int hold, const atc_state_t* st, const float* actions,
                       const atc_out_t* out, const atc_params_t* p, void* stream) {
    if (!actions || !out) return fail_arg("null pointer");
    if (const int rc = check_env_args(s, B, N, st, p)) return rc;
    if (T < 1 || hold < 1) return fail_arg("need T >= 1 and hold >= 1");
    // actions is [T / hold] blocks: a partial last block would be read beyond what the header promises exists
    if (T % hold != 0) return fail_arg("T must be a multiple of hold (actions holds T / hold blocks)");
    if (const int rc = check_required_outputs(out)) return rc;
    if (out->packet && (N != 1 || T != 1)) return fail_arg("atc_out_t.packet is for single steps of single-aircraft envs");
    if (const int rc = check_dt(s, p)) return rc;
    return with_width(N, [&](auto w) { return launch_step<decltype(w)::value>(s, B, N, T, hold, st, actions, out, p, (hipStream_t)stream); });
}

// ---- frame skip (include/atc_step.h: atc_step_skip) ------------------------------------------------------------------------------
template <int W>
static int launch_skip(const atc_scenario* s, int B, int N, int K, const atc_state_t* st, const float* actions, const atc_out_t* out,
                       uint8_t* n_steps, const atc_params_t* p, hipStream_t stream) {
    const size_t lds = lds_bytes(s, W >= 32, true);
    const int grid = step_grid(B, W);
    const StepDerived& q = derive(*p, s, 0);
    // as for k_step: a launch that asks for no optional output runs the form that has them compiled out
    return with_flag(out->raw_obs || out->ac_reward || out->min_sep || out->term_obs, [&](auto full) {
        hipLaunchKernelGGL((k_skip<W, decltype(full)::value>), dim3(grid), dim3(kBlock), lds, stream, s->d_blob, s->off_grid, B, N, K, 0, *st, actions, *out, *p, q, n_steps);
        HIP_TRY(hipGetLastError());
        ++record(REC_SKIP)[__builtin_ctz(W)];
        return ATC_OK;
    });
}

// ---- traffic observation (include/atc_step.h: atc_observe_traffic) -------------------------------------------------------------
// the uniform terms of a traffic query (TrafficArgs): atc_observe_traffic's, and the policy rollout's that takes the query inside its launch
static TrafficArgs traffic_common(const atc_scenario* s, const atc_params_t* p, int K) {
    TrafficArgs q;
    q.pos_inv = (double)s->consts[ATC_C_POS_INV];
    q.x0 = (double)s->consts[ATC_C_POS_X0];
    q.y0 = (double)s->consts[ATC_C_POS_Y0];
    const bool nrm = (p->mode & ATC_M_NORMALIZE) != 0;
    q.s_pos = nrm ? 1.0f / s->consts[ATC_C_WORLD_DIAG] : 1.0f;
    q.h_div = nrm ? s->consts[ATC_C_H_MAX] : 1.0f;
    q.s_v = nrm ? 1.0f / (2.0f * s->consts[ATC_C_V_MAX]) : 1.0f;
    q.K = K;
    return q;
}
template <int W, int KT>
static int launch_traffic2(int B, int N, const atc_state_t* st, float* traffic, const TrafficArgs& q, hipStream_t stream) {
    hipLaunchKernelGGL((k_traffic<W, KT>), dim3(step_grid(B, W)), dim3(kBlock), 0, stream, B, N, *st, traffic, q);
    HIP_TRY(hipGetLastError());
    ++record(REC_TRAFFIC)[__builtin_ctz(W)];
    return ATC_OK;
}
// the compiled list lengths are 1, 2, 4, 8: a K in between runs the next one and stores its first K records
template <int W>
static int launch_traffic(int B, int N, const atc_state_t* st, float* traffic, const TrafficArgs& q, hipStream_t stream) {
    if (q.K == 1) return launch_traffic2<W, 1>(B, N, st, traffic, q, stream);
    if (q.K == 2) return launch_traffic2<W, 2>(B, N, st, traffic, q, stream);
    if (q.K <= 4) return launch_traffic2<W, 4>(B, N, st, traffic, q, stream);
    return launch_traffic2<W, 8>(B, N, st, traffic, q, stream);
}

// ---- the candidate kernels (include/atc_step.h: atc_lookahead, atc_lookahead_plan, atc_lookahead_plan_sampled, atc_branch) ----------
// candidates per workgroup (csrc/atc_lookahead.inc) asked for by atc_lookahead_set_mapping; 0: the library's choice
static thread_local int t_look_cpg = 0;
#define ATC_LOOKAHEAD_CPG_DEFAULT 1   // one workgroup per (tile, candidate): measured against the in-workgroup loop in DESIGN.md, section 3c

// the launch shape k_lookahead and k_plan share: 256-slot tiles of the batch x groups of `cpg` candidates (atc_lookahead_set_mapping)
struct CandGrid {
    int tiles, cpg, groups;
    unsigned grid;
};
static int cand_grid(int B, int W, int M, CandGrid* g) {
    g->tiles = step_grid(B, W);
    g->cpg = std::min(t_look_cpg > 0 ? t_look_cpg : ATC_LOOKAHEAD_CPG_DEFAULT, M);
    g->groups = (M + g->cpg - 1) / g->cpg;
    const long long grid = (long long)((g->tiles + 7) / 8) * 8 * g->groups;   // whole chunks of 8 tiles x groups (look_tile)
    if (grid > 0x7fffffffll) return fail_arg("B*N*M too large for one launch: split the candidates");
    g->grid = (unsigned)grid;
    return ATC_OK;
}
// the kernels' atc_out_t from the six fields atc_lookahead_out_t and atc_plan_out_t name alike
template <typename O>
static atc_out_t cand_out(const O* o) {
    atc_out_t out;
    memset(&out, 0, sizeof out);
    out.obs = o->obs; out.reward = o->reward; out.ac_reward = o->ac_reward; out.done = o->done; out.flags = o->flags; out.min_sep = o->min_sep;
    return out;
}
// true: one of the four optional outputs is asked for (the look-ahead kernels' fast form has them compiled out)
template <typename O>
static bool cand_any(const O* o) {
    return o->flags || o->ac_reward || o->min_sep || o->obs;
}
// The one launch of the candidate kernels (k_lookahead, k_plan, k_plan_sampled, k_branch, k_lookahead_policy): the grid, the kernels' atc_out_t, the derived
// constants, then `launch(w, full, g, lds, out, q)` — the caller's generic lambda, which names the kernel instantiation
// <decltype(w)::value, decltype(full)::value> and its argument list — and the count in record `rec`, slot log2(W).  `any` picks the
// form with the optional outputs compiled in: cand_any(o), or atc_branch's own rule.
template <typename O, typename L>
static int launch_candidates(Record rec, const atc_scenario* s, int B, int N, int M, const O* o, bool any, const atc_params_t* p, L launch) {
    return with_width(N, [&](auto w) {
        constexpr int W = decltype(w)::value;
        CandGrid g;
        if (const int rc = cand_grid(B, W, M, &g)) return rc;
        const atc_out_t out = cand_out(o);
        const StepDerived& q = derive(*p, s, 0);
        return with_flag(any, [&](auto full) {
            launch(w, full, g, lds_bytes(s, W >= 32, true), out, q);
            HIP_TRY(hipGetLastError());
            ++record(rec)[__builtin_ctz(W)];
            return ATC_OK;
        });
    });
}

// ---- argument checks of the candidate and drawn-plan calls ----------------------------------------------------------------------
static int check_plan_h(int H) {
    if (H < 1 || H > ATC_PLAN_MAX_H) return fail_arg("H (the number of segments of a plan) must be 1 .. 16");
    return ATC_OK;
}
static int check_drawn_m(int M) {
    if (M < 1 || M > ATC_SAMPLE_MAX_M) return fail_arg("M (the number of drawn candidates) must be 1 .. 1024");
    return ATC_OK;
}
static int check_continuous(const atc_params_t* p) {
    if (p->mode & ATC_M_DISCRETE) return fail_arg("ATC_M_DISCRETE: only the continuous action space is drawn");
    return ATC_OK;
}
// a pointer a call requires and the words it is refused in when null; a list of them is looked at in its order
struct Required { const void* ptr; const char* refusal; };
static int check_required(std::initializer_list<Required> list) {
    for (const Required& r : list)
        if (!r.ptr) return fail_arg(r.refusal);
    return ATC_OK;
}
// the pointers more than one drawn-plan call requires: the three sources of a drawn plan (include/atc_step.h:
// atc_lookahead_plan_sampled) and the candidates' weights
static Required need_mean(const float* mean) { return {mean, "null pointer: mean is required"}; }
static Required need_std(const float* std) { return {std, "null pointer: std is required"}; }
static Required need_dr(const atc_plan_draw_t* dr) { return {dr, "null pointer: dr (atc_plan_draw_t) is required"}; }
static Required need_weight(const float* weight) { return {weight, "null pointer: weight is required"}; }
// The checks of atc_plan_draw, atc_plan_refit and atc_plan_score up to the batch shape: H, then M, then the call's further count
// (`count_refusal`: null, or what is wrong with E / R), all before any pointer is looked at; then the required pointers in the caller's
// order; then, for a call that has parameters (`p`, itself among `required`; atc_plan_score has neither p nor N, and goes on with
// checks of its own), the continuous action space and the batch shape.
static int check_drawn_plan(int H, int M, const char* count_refusal, std::initializer_list<Required> required, const atc_params_t* p = nullptr,
                            int B = 0, int N = 0) {
    if (const int rc = check_plan_h(H)) return rc;
    if (const int rc = check_drawn_m(M)) return rc;
    if (count_refusal) return fail_arg(count_refusal);
    if (const int rc = check_required(required)) return rc;
    if (!p) return ATC_OK;
    if (const int rc = check_continuous(p)) return rc;
    if (const int rc = check_batch_range(B, N)) return rc;
    return check_batch_size(B, N);
}
// the argument checks of atc_lookahead (H null), atc_lookahead_plan and atc_lookahead_plan_sampled (`drawn`: dr, mean, std in place of
// `actions`): K, then H, then M, before any pointer is looked at
template <typename O>
static int check_candidates(const atc_scenario_t* s, int B, int N, int K, const int* H, int M, const atc_state_t* st, const float* actions,
                            const O* out, const atc_params_t* p, const char* k_is, const char* out_type, const char* fresh_per,
                            std::initializer_list<Required> drawn = {}) {
    const bool is_drawn = drawn.size() != 0;
    if (K < 1 || K > ATC_SKIP_MAX) return fail_argf("K (the %s length) must be 1 .. 255", k_is);
    if (H) if (const int rc = check_plan_h(*H)) return rc;
    if (is_drawn) {
        if (const int rc = check_drawn_m(M)) return rc;
        if (const int rc = check_required(drawn)) return rc;
    } else if (M < 1 || M > ATC_LOOKAHEAD_MAX_M) return fail_arg("M (the number of candidates) must be 1 .. 64");
    if (!out || !out->reward || !out->done) return fail_argf("null pointer: %s.reward and .done are required", out_type);
    if (!is_drawn && !actions) return fail_arg("null pointer");
    if (const int rc = check_env_args(s, B, N, st, p)) return rc;
    if (const int rc = check_dt(s, p)) return rc;
    if (p->mode & ATC_M_ACTIONS_HELD) return fail_argf("ATC_M_ACTIONS_HELD is for atc_step only: every %s's first step carries a fresh decision", fresh_per);
    return is_drawn ? check_continuous(p) : ATC_OK;
}

// ---- byte ranges that must not share memory (atc_plan_refit, atc_plan_score, atc_branch, atc_state_select, atc_gae) ---------------------
// Pointer VALUES only: nothing is dereferenced.  Ranges that only touch do not overlap.
struct ByteRange { const void* ptr; uintptr_t bytes; const char* name; };
static bool ranges_overlap(const ByteRange& a, const ByteRange& b) {
    const uintptr_t alo = reinterpret_cast<uintptr_t>(a.ptr), blo = reinterpret_cast<uintptr_t>(b.ptr);
    return alo < blo + b.bytes && blo < alo + a.bytes;
}
// every pair of r[0 .. n-1], null entries left out; a pair listed in `may_equal` (first < second) is let through as EQUAL pointers (an
// in-place update).  Refused as "<name> overlaps <name> (<tail>)".
static int check_disjoint(const ByteRange* r, int n, std::initializer_list<std::pair<int, int>> may_equal, const char* tail) {
    for (int a = 0; a < n; ++a)
        for (int b = a + 1; b < n; ++b) {
            if (!r[a].ptr || !r[b].ptr || !ranges_overlap(r[a], r[b])) continue;
            bool in_place = false;
            for (const auto& pair : may_equal) in_place |= pair.first == a && pair.second == b && r[a].ptr == r[b].ptr;
            if (in_place) continue;
            return fail_argf("%s overlaps %s (%s)", r[a].name, r[b].name, tail);
        }
    return ATC_OK;
}
// true if any of the six arrays of `a` (Ba envs x N aircraft) shares a byte with any array of `b` (Bb envs)
static bool states_overlap(const atc_state_t* a, unsigned long long Ba, const atc_state_t* b, unsigned long long Bb, unsigned long long N) {
    auto ranges = [N](const atc_state_t* st, unsigned long long B, ByteRange r[6]) {
        const void* ptr[6] = {st->ac, st->alt, st->last_act, st->env, st->stats, st->phi_wide};
        const unsigned long long bytes[6] = {B * N * 16ull, B * N * 8ull, B * N * 16ull, B * (ATC_ENV_WORDS * 4ull), B * (ATC_STAT_WORDS * 4ull), B * N * 32ull};
        for (int i = 0; i < 6; ++i) r[i] = ByteRange{ptr[i], (uintptr_t)bytes[i], nullptr};
    };
    ByteRange ra[6], rb[6];
    ranges(a, Ba, ra);
    ranges(b, Bb, rb);
    for (int i = 0; i < 6; ++i)
        for (int j = 0; j < 6; ++j)
            if (ranges_overlap(ra[i], rb[j])) return true;
    return false;
}

// ---- policy rollout (include/atc_step.h: atc_rollout_policy, atc_rollout_policy_traffic) ----------------------------------------------
// the kernels' atc_out_t from the four step outputs atc_policy_out_t and atc_policy_traffic_out_t name alike
template <typename O>
static atc_out_t policy_out(const O* o) {
    atc_out_t out;
    memset(&out, 0, sizeof(out));
    out.obs = o->obs;
    out.reward = o->reward;
    out.done = o->done;
    out.flags = o->flags;
    return out;
}
// W lanes per env.  KT = 0: k_rollout_policy (P, O = atc_policy_t, atc_policy_out_t); KT = 1, 2, 4: k_rollout_policy_traffic<W, KT>, whose
// selection borrows the pair-scan staging area between steps at W >= 32 (P, O = atc_policy_traffic_t, atc_policy_traffic_out_t).
// ENDS: k_rollout_policy_ends<W, KT> for KT = 0, 1, 2, 4 (P, O = atc_policy_traffic_t, atc_policy_ends_out_t)
// TERM (with ENDS): k_rollout_policy_term<W, KT> for KT = 1, 2, 4 (O = atc_policy_term_out_t)
template <int W, int KT, bool ENDS = false, bool TERM = false, typename P, typename O>
static int launch_policy(const atc_scenario* s, int B, int N, int T, int hold, const atc_state_t* st, const float* obs0, const P* pol, const O* o,
                         const atc_params_t* p, hipStream_t stream) {
    const size_t lds = lds_bytes(s, W >= 32, true);
    const int grid = step_grid(B, W);
    const StepDerived& q = derive(*p, s, 0);
    auto launch = [&](auto kernel, auto... tail) {
        hipLaunchKernelGGL(kernel, dim3(grid), dim3(kBlock), lds, stream, s->d_blob, s->off_grid, B, N, T, hold, *st, obs0, policy_out(o), *p, q, pol->w, pol->seed,
                           pol->decision0, pol->flags, o->action, o->logp, tail...);
    };
    uint64_t* rec;
    if constexpr (TERM) {
        static_assert(ENDS && KT > 0, "the terminal records belong to the ends of a policy that sees traffic");
        launch(k_rollout_policy_term<W, KT>, PolicyTrafficTail{traffic_common(s, p, KT), o->traffic}, PolicyEnds{o->term_obs, o->term_flags, o->control},
               PolicyTerm{o->term_traffic});
        rec = &record(REC_POLICY_TERM)[3 * __builtin_ctz(W) + __builtin_ctz(KT)];
    } else if constexpr (ENDS) {
        launch(k_rollout_policy_ends<W, KT>, PolicyTrafficTail{KT ? traffic_common(s, p, KT) : TrafficArgs{}, o->traffic}, PolicyEnds{o->term_obs, o->term_flags, o->control});
        rec = &record(REC_POLICY_ENDS)[4 * __builtin_ctz(W) + (KT ? 1 + __builtin_ctz(KT) : 0)];
    } else if constexpr (KT == 0) {
        launch(k_rollout_policy<W>);
        rec = &record(REC_POLICY)[__builtin_ctz(W)];
    } else {
        launch(k_rollout_policy_traffic<W, KT>, PolicyTrafficTail{traffic_common(s, p, KT), o->traffic});
        rec = &record(REC_POLICY_TRAFFIC)[3 * __builtin_ctz(W) + __builtin_ctz(KT)];
    }
    HIP_TRY(hipGetLastError());
    ++*rec;
    return ATC_OK;
}
// f(std::integral_constant<int, KT>) for a checked atc_policy_traffic_t.traffic_k: the compiled list lengths 1, 2, 4
template <typename F>
static int with_traffic_k(int k, F f) {
    if (k == 1) return f(std::integral_constant<int, 1>());
    if (k == 2) return f(std::integral_constant<int, 2>());
    return f(std::integral_constant<int, 4>());
}
// atc_policy_eval's launch: k_policy_eval<W, KT> for KT = 0, 1, 2, 4 on launch_policy's grid, its out, action and logp parameters zero
template <int W, int KT>
static int launch_policy_eval(const atc_scenario* s, int B, int N, int T, int hold, const atc_state_t* st, const float* obs0, const atc_policy_traffic_t* pol,
                              const atc_policy_eval_out_t* o, const atc_params_t* p, hipStream_t stream) {
    atc_out_t none;
    memset(&none, 0, sizeof(none));
    hipLaunchKernelGGL((k_policy_eval<W, KT>), dim3(step_grid(B, W)), dim3(kBlock), lds_bytes(s, W >= 32, true), stream, s->d_blob, s->off_grid, B, N, T, hold, *st, obs0,
                       none, *p, derive(*p, s, 0), pol->w, pol->seed, pol->decision0, pol->flags, (float*)nullptr, (float*)nullptr,
                       PolicyTrafficTail{KT ? traffic_common(s, p, KT) : TrafficArgs{}, nullptr}, PolicyEval{o->record, o->obs_last, o->flags});
    HIP_TRY(hipGetLastError());
    ++record(REC_POLICY_EVAL)[4 * __builtin_ctz(W) + (KT ? 1 + __builtin_ctz(KT) : 0)];
    return ATC_OK;
}
// ... and for atc_rollout_policy_ends, whose traffic_k may also be 0 (the ten-word policy)
template <typename F>
static int with_traffic_k0(int k, F f) {
    return k == 0 ? f(std::integral_constant<int, 0>()) : with_traffic_k(k, f);
}

// The argument checks of the policy launches (the three rollouts and atc_policy_eval), in the header's order, in three parts: what is
// refused up to `out` itself (policy_call_head), the call's own required outputs (at the caller), what is refused from n_hidden to the mode
// (policy_call_env), then the call's own tail — the overlap rule of the rollouts (check_policy_call) or atc_policy_eval's two refusals
// and its overlap rule (check_policy_eval_call).  `out_type` names the output struct in the refusals; traffic_k is null for
// atc_rollout_policy; `k0`: traffic_k may be 0, the ten-word policy (atc_rollout_policy_ends, atc_policy_eval) — then `traffic` must be NULL.
template <typename P>
static int policy_call_head(int T, int hold, const float* obs0, const P* pol, const void* out, const char* pol_type, const char* out_type) {
    // T and hold first, before any pointer is looked at
    if (T < 1 || hold < 1) return fail_arg("need T >= 1 and hold >= 1");
    if (T % hold != 0) return fail_arg("T must be a multiple of hold (the launch takes T / hold decisions)");
    if (!pol) return fail_argf("null pointer: pol (%s) is required", pol_type);
    if (const int rc = check_required({{pol->w, "null pointer: pol->w (the policy's weights) is required"}, {obs0, "null pointer: obs0 is required"}})) return rc;
    if (!out) return fail_argf("null pointer: out (%s) is required", out_type);
    return ATC_OK;
}
// `dt`: false leaves the time increment, the one refusal that reads the sector, to the caller (atc_rollout_policy_term makes it last).
template <typename P>
static int policy_call_env(const atc_scenario_t* s, int B, int N, const atc_state_t* st, const P* pol, const atc_params_t* p, const char* out_type,
                           const int32_t* traffic_k, const float* traffic, bool k0, bool dt = true) {
    if (pol->n_hidden != ATC_POLICY_HIDDEN) return fail_arg("pol->n_hidden must be 64 (ATC_POLICY_HIDDEN)");
    if (traffic_k && !(k0 && *traffic_k == 0) && *traffic_k != 1 && *traffic_k != 2 && *traffic_k != 4)
        return fail_arg(k0 ? "pol->traffic_k must be 0, 1, 2 or 4 (the ten-word policy, or a compiled list length)" : "pol->traffic_k must be 1, 2 or 4 (the compiled list lengths)");
    if (pol->flags & ~ATC_POLICY_DETERMINISTIC) return fail_arg("pol->flags has unknown bits (ATC_POLICY_DETERMINISTIC or 0)");
    if (k0 && *traffic_k == 0 && traffic) return fail_argf("%s.traffic must be NULL where pol->traffic_k is 0 (no traffic query is evaluated)", out_type);
    if (const int rc = check_env_args(s, B, N, st, p)) return rc;
    if (dt) if (const int rc = check_dt(s, p)) return rc;
    if (p->mode & ATC_M_DISCRETE) return fail_arg("ATC_M_DISCRETE: a Gaussian policy draws the continuous action space only");
    if (p->mode & ATC_M_ACTIONS_HELD) return fail_arg("ATC_M_ACTIONS_HELD is for atc_step only: every block's first step carries a fresh decision");
    return ATC_OK;
}
// `w` against each of others[0 .. n-1] (NULL entries left out), refused with `tail`
static int check_apart(const ByteRange& w, const ByteRange* others, int n, const char* tail) {
    for (int i = 0; i < n; ++i) {
        const ByteRange pair[2] = {w, others[i]};
        if (const int rc = check_disjoint(pair, 2, {}, tail)) return rc;
    }
    return ATC_OK;
}
// the three rollouts.  `traffic` is atc_policy_traffic_out_t.traffic (its range joins the overlap rule); `ends`: the call is
// atc_rollout_policy_ends, whose three arrays join the overlap rule.  `term`: the call is atc_rollout_policy_term — traffic_k == 0 is refused
// as by atc_rollout_policy_traffic, and the time increment is left to check_policy_term_call.
template <typename P, typename O>
static int check_policy_call(const atc_scenario_t* s, int B, int N, int T, int hold, const atc_state_t* st, const float* obs0, const P* pol, const O* out,
                             const atc_params_t* p, const char* pol_type, const char* out_type, const int32_t* traffic_k, const float* traffic,
                             const PolicyEnds* ends = nullptr, bool term = false) {
    if (const int rc = policy_call_head(T, hold, obs0, pol, out, pol_type, out_type)) return rc;
    if (!out->obs || !out->reward || !out->done || !out->flags) return fail_argf("null pointer: %s.obs, .reward, .done and .flags are required", out_type);
    if (!out->action) return fail_argf("null pointer: %s.action is required", out_type);
    if (const int rc = policy_call_env(s, B, N, st, pol, p, out_type, traffic_k, traffic, ends != nullptr && !term, !term)) return rc;
    const uintptr_t bn = (uintptr_t)B * (uintptr_t)N, row = bn * (ATC_OBS_DIM * 4u), n_dec = (uintptr_t)(T / hold);
    const ByteRange ranges[2] = {{obs0, row, "obs0"}, {out->obs, row * (uintptr_t)T, "out->obs"}};
    if (const int rc = check_disjoint(ranges, 2, {}, "decision 0 reads obs0 while the steps write out->obs")) return rc;
    // ... and what is written per decision (NULL: left out): against what the launch reads or writes next to it, and against one another
    const ByteRange per_decision[4] = {{traffic, traffic ? n_dec * bn * (uintptr_t)*traffic_k * (ATC_TRAFFIC_DIM * 4u) : 0u, "out->traffic"},
                                       {ends ? ends->term_obs : nullptr, n_dec * row, "out->term_obs"},
                                       {ends ? ends->term_flags : nullptr, n_dec * (uintptr_t)B * 2u, "out->term_flags"},
                                       {ends ? ends->control : nullptr, n_dec * bn, "out->control"}};
    for (int w = 0; w < 4; ++w) {
        if (!per_decision[w].ptr) continue;
        ByteRange others[11] = {ranges[0], ranges[1], {st->ac, bn * 16u, "st->ac"}, {st->alt, bn * 8u, "st->alt"}, {st->last_act, bn * 16u, "st->last_act"},
                                {st->env, (uintptr_t)B * (ATC_ENV_WORDS * 4u), "st->env"}, {st->stats, (uintptr_t)B * (ATC_STAT_WORDS * 4u), "st->stats"},
                                {st->phi_wide, bn * 32u, "st->phi_wide"}};
        int n = 8;
        for (int v = 0; v < w; ++v) others[n++] = per_decision[v];
        if (const int rc = check_apart(per_decision[w], others, n, w == 0 ? "the records are written while the launch reads and writes the other"
                                                                          : "it is written while the launch reads and writes the other"))
            return rc;
    }
    return ATC_OK;
}
// atc_rollout_policy_term: atc_rollout_policy_ends' refusals in its order (traffic_k outside {1, 2, 4} refused where it refuses its own), then
// term_traffic against the weights, obs0, every other output and the six state arrays, then the time increment — last, since it alone
// reads the sector: everything in front of it follows no pointer but pol, out, st and p.
static int check_policy_term_call(const atc_scenario_t* s, int B, int N, int T, int hold, const atc_state_t* st, const float* obs0, const atc_policy_traffic_t* pol,
                                  const atc_policy_term_out_t* out, const atc_params_t* p) {
    const PolicyEnds ends = {out ? out->term_obs : nullptr, out ? out->term_flags : nullptr, out ? out->control : nullptr};
    if (const int rc = check_policy_call(s, B, N, T, hold, st, obs0, pol, out, p, "atc_policy_traffic_t", "atc_policy_term_out_t", pol ? &pol->traffic_k : nullptr,
                                         out ? out->traffic : nullptr, &ends, true))
        return rc;
    if (out->term_traffic) {
        const uintptr_t b = (uintptr_t)B, bn = b * (uintptr_t)N, row = bn * (ATC_OBS_DIM * 4u), t = (uintptr_t)T, n_dec = (uintptr_t)(T / hold), k = (uintptr_t)pol->traffic_k;
        const ByteRange records = {out->term_traffic, n_dec * bn * k * (ATC_TRAFFIC_DIM * 4u), "out->term_traffic"};
        const ByteRange others[18] = {{pol->w, (uintptr_t)ATC_POLICY_TRAFFIC_WORDS(pol->traffic_k) * 4u, "pol->w"}, {obs0, row, "obs0"}, {out->obs, row * t, "out->obs"},
                                      {out->reward, t * b * 4u, "out->reward"}, {out->done, t * b, "out->done"}, {out->flags, t * bn * 2u, "out->flags"},
                                      {out->action, n_dec * bn * 12u, "out->action"}, {out->logp, n_dec * bn * 4u, "out->logp"},
                                      {out->traffic, n_dec * bn * k * (ATC_TRAFFIC_DIM * 4u), "out->traffic"}, {out->term_obs, n_dec * row, "out->term_obs"},
                                      {out->term_flags, n_dec * b * 2u, "out->term_flags"}, {out->control, n_dec * bn, "out->control"},
                                      {st->ac, bn * 16u, "st->ac"}, {st->alt, bn * 8u, "st->alt"}, {st->last_act, bn * 16u, "st->last_act"},
                                      {st->env, b * (ATC_ENV_WORDS * 4u), "st->env"}, {st->stats, b * (ATC_STAT_WORDS * 4u), "st->stats"}, {st->phi_wide, bn * 32u, "st->phi_wide"}};
        if (const int rc = check_apart(records, others, 18, "the terminal records are written while the launch reads and writes the other")) return rc;
    }
    return check_dt(s, p);
}
// atc_policy_eval: out->record stands where the rollouts' required outputs do; behind the mode's refusals its own two; record and obs_last
// against obs0, the six state arrays and each other.
static int check_policy_eval_call(const atc_scenario_t* s, int B, int N, int T, int hold, const atc_state_t* st, const float* obs0, const atc_policy_traffic_t* pol,
                                  const atc_policy_eval_out_t* out, const atc_params_t* p) {
    const char* const out_type = "atc_policy_eval_out_t";
    if (const int rc = policy_call_head(T, hold, obs0, pol, out, "atc_policy_traffic_t", out_type)) return rc;
    if (!out->record) return fail_argf("null pointer: %s.record is required", out_type);
    if (const int rc = policy_call_env(s, B, N, st, pol, p, out_type, &pol->traffic_k, nullptr, true)) return rc;
    // (the step forms the per-episode words k_policy_eval reads back only on its auto-reset path)
    if (!(p->mode & ATC_M_AUTO_RESET)) return fail_arg("ATC_M_AUTO_RESET is required: an evaluation counts episodes, which end and restart inside the step");
    if (out->flags & ~ATC_EVAL_CLEAR) return fail_argf("%s.flags has unknown bits (ATC_EVAL_CLEAR or 0)", out_type);
    const uintptr_t bn = (uintptr_t)B * (uintptr_t)N, row = bn * (ATC_OBS_DIM * 4u);
    const ByteRange record = {out->record, (uintptr_t)B * (ATC_EVAL_WORDS * 4u), "out->record"};
    const ByteRange others[8] = {{out->obs_last, row, "out->obs_last"}, {obs0, row, "obs0"}, {st->ac, bn * 16u, "st->ac"}, {st->alt, bn * 8u, "st->alt"},
                                 {st->last_act, bn * 16u, "st->last_act"}, {st->env, (uintptr_t)B * (ATC_ENV_WORDS * 4u), "st->env"},
                                 {st->stats, (uintptr_t)B * (ATC_STAT_WORDS * 4u), "st->stats"}, {st->phi_wide, bn * 32u, "st->phi_wide"}};
    const char* const tail = "it is written while the launch reads and writes the other";
    if (const int rc = check_apart(record, others, 8, tail)) return rc;
    return check_apart(others[0], others + 1, 7, tail);
}

#include "atc_abi.inc"   // the extern "C" entry points (host side)
