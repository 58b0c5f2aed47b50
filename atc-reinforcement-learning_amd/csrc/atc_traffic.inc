// atc_traffic.inc — k_traffic, the kernel of atc_observe_traffic (include/atc_step.h: "Traffic observation"): for every aircraft the
// K nearest other aircraft under control in its env, nearest first, as 8-word records in the observing aircraft's own frame.
// Included by atc_step.hip next to atc_aux_kernels.inc (one translation unit, the per-lane device functions of atc_device.h and the
// DPP helpers of atc_wave.h).  Reads state only; the step kernels know nothing of it.  The arithmetic behind its loads (traffic_self,
// traffic_select, traffic_record) is shared with k_rollout_policy_traffic (atc_policy.inc), which evaluates it on the state in registers.
//
// Mapping: one lane per aircraft slot, groups of W = next_pow2(N) lanes per env, 256 slots per workgroup — k_step's.  An env never
// straddles a wavefront (W <= 64), so every partner of a lane lives in its own wavefront:
//   selection  every lane sees each other slot of its env once — (x, y, tag) arrive through DPP operand modifiers for W <= 16 (the
//              partners of the scans in atc_wave.h: XOR partners inside a quad / half row, row rotations for W = 16) and from an LDS
//              copy for W = 32, 64 (all lanes of a group read the same word: a broadcast, no bank conflict) — and keeps its KT best
//              64-bit keys  (bits of d2) << 32 | slot  sorted in registers by compare-exchange insertion.  d2 >= 0 and finite, so its
//              bit pattern orders it; the slot in the low word makes ties go to the lower slot whatever order the partners arrive in.
//              A partner that is idle, beyond the batch or not under control carries tag -1 and offers the key ~0, which no real key
//              reaches: it never displaces anything, and a rank that still holds ~0 afterwards is an ABSENT record.
//   features   per kept record the winner's x, y, h and ground velocity are fetched by lane index (ds_bpermute) — five words per
//              record kept, not per partner seen — and rotated into the observer's frame.
//   store      a lane's K records are 32 K contiguous bytes: 2 K 16-byte stores.
// KT (1, 2, 4, 8) is the compiled list length; a call with K in between runs the next KT and stores the first K records.

// sin / cos of the heading 180 + phi_fix 2^-23 deg: the kinematics' float64 reduction and polynomials (include/atc_step.h "Heading
// kinematics"; advance() in atc_device.h negates the DISTANCE for an even k — the same sign, here on the pair itself)
__device__ __forceinline__ void heading_sincos(int phi_fix, float& sn, float& cs) {
    const double pd = (double)phi_fix;
    const double kd = __builtin_rint(pd * ATC_KIN_INV180);
    const double t = __builtin_fma(kd, -ATC_KIN_HALF_TURN, pd);
    const double u = t * t;
    double sp = __builtin_fma(u, ATC_KIN_S5, ATC_KIN_S4), cp = __builtin_fma(u, ATC_KIN_C5, ATC_KIN_C4);
    sp = __builtin_fma(sp, u, ATC_KIN_S3);
    cp = __builtin_fma(cp, u, ATC_KIN_C3);
    sp = __builtin_fma(sp, u, ATC_KIN_S2);
    cp = __builtin_fma(cp, u, ATC_KIN_C2);
    sp = __builtin_fma(sp, u, ATC_KIN_S1);
    cp = __builtin_fma(cp, u, ATC_KIN_C1);
    sp = __builtin_fma(sp, u, ATC_KIN_S0);
    const double c = __builtin_fma(cp, u, 1.0), s = sp * t;
    const bool even = (cvt_i32_f64(kd) & 1) == 0;   // phi = 180 (1 + k) + t: an even k is an odd number of half turns
    sn = (float)(even ? -s : s);
    cs = (float)(even ? -c : c);
}

// developer switch (build.py's `extra` flags): 1 stores the records non-temporal.  Measured, not adopted (faster for K = 1 only, DESIGN.md 3b): profiles/traffic_bench_nt_stores.json
#ifndef ATC_TRAFFIC_NT_STORES
#define ATC_TRAFFIC_NT_STORES 0
#endif

struct TrafficArgs {      // uniform terms, evaluated on the host (traffic_common)
    double pos_inv, x0, y0;   // position grid: nm = origin + counts * 2^-k
    float s_pos, s_v, h_div;  // ATC_M_NORMALIZE: 1 / world diagonal, 1 / (2 v_max), h_max; 1 otherwise.  The altitude difference is
                              // exact, so its scaled form is the correctly rounded quotient; the other words are values (1e-5)
    int K;                    // records stored per aircraft (<= KT)
};

constexpr uint64_t kTrafficNone = ~0ull;

template <int KT>
__device__ __forceinline__ void traffic_insert(uint64_t (&best)[KT], uint64_t c) {
#pragma unroll
    for (int r = 0; r < KT; ++r) {   // compare-exchange down the sorted list: the smaller key stays, the larger one moves on
        const uint64_t b = best[r];
        const bool lt = c < b;
        best[r] = lt ? c : b;
        c = lt ? b : c;
    }
}
template <int KT>
__device__ __forceinline__ void traffic_offer(uint64_t (&best)[KT], float x, float y, float px, float py, int ptag) {
    const float dx = px - x, dy = py - y;
    const float d2 = fmaf(dx, dx, dy * dy);   // the separation scan's expression
    const uint64_t key = ((uint64_t)__float_as_uint(d2) << 32) | (uint32_t)ptag;
    traffic_insert<KT>(best, ptag < 0 ? kTrafficNone : key);
}
template <int CTRL>
__device__ __forceinline__ int dpp_i(int v) {
    return __builtin_amdgcn_update_dpp(0, v, CTRL, 0xf, 0xf, false);
}
template <int KT, int CTRL>
__device__ __forceinline__ void traffic_offer_dpp(uint64_t (&best)[KT], float x, float y, float sx, float sy, int stag) {
    traffic_offer<KT>(best, x, y, dpp_f<CTRL>(sx), dpp_f<CTRL>(sy), dpp_i<CTRL>(stag));   // the partner's copy of (sx, sy, stag)
}
template <int KT, int D>
struct TrafficRow16 {   // W = 16: row rotations 1 .. 15 visit every other lane of the row once
    static __device__ __forceinline__ void run(uint64_t (&best)[KT], float x, float y, int tag) {
        traffic_offer_dpp<KT, 0x120 + D>(best, x, y, x, y, tag);
        TrafficRow16<KT, D + 1>::run(best, x, y, tag);
    }
};
template <int KT>
struct TrafficRow16<KT, 16> {
    static __device__ __forceinline__ void run(uint64_t (&)[KT], float, float, int) {}
};

// ---- the arithmetic behind the loads, shared by k_traffic and k_rollout_policy_traffic (atc_policy.inc): the file is built with
// -ffp-contract=off, so both callers produce the same bits ---------------------------------------------------------------------------
struct TrafficSelf {      // what a lane offers its partners and rotates their records with
    float x, y, h, vx, vy, sn, cs;
};
// from the state words of one aircraft; `phi` is the heading's counts, a WIDE one already wrapped (phi_wrap of the side record)
__device__ __forceinline__ TrafficSelf traffic_self(int px, int py, double alt, int phi, uint32_t v_fix, const TrafficArgs& q) {
    TrafficSelf me;
    me.x = (float)__builtin_fma((double)px, q.pos_inv, q.x0);
    me.y = (float)__builtin_fma((double)py, q.pos_inv, q.y0);
    me.h = (float)alt;
    heading_sincos(phi, me.sn, me.cs);
    const float v = v_real(v_fix);
    me.vx = v * me.sn;
    me.vy = v * me.cs;
    return me;
}

// selection: the KT best keys of lane k (tag = k under control, -1 otherwise) over the other slots of its group of W lanes.  W >= 32
// reads the partners from LDS: sx / sy / stag point at the GROUP's first slot, written by every lane of the group and ordered by the
// caller (k_traffic: a workgroup barrier; the policy rollout: wave-level waits on its wavefront's own slice); unused below 32.
template <int W, int KT>
__device__ __forceinline__ void traffic_select(uint64_t (&best)[KT], float x, float y, int tag, int k, int N, const float* sx, const float* sy,
                                               const int* stag) {
#pragma unroll
    for (int r = 0; r < KT; ++r) best[r] = kTrafficNone;
    if constexpr (W >= 32) {
        for (int j = 0; j < N; ++j) {
            const int pt = stag[j];
            traffic_offer<KT>(best, x, y, sx[j], sy[j], pt == k ? -1 : pt);
        }
    } else if constexpr (W == 16) {
        TrafficRow16<KT, 1>::run(best, x, y, tag);
    } else if constexpr (W >= 2) {
        constexpr int X1 = 0xB1, X2 = 0x4E, X3 = 0x1B, HALF_MIRROR = 0x141;   // (atc_wave.h: pair_scan_xor)
        traffic_offer_dpp<KT, X1>(best, x, y, x, y, tag);
        if constexpr (W >= 4) {
            traffic_offer_dpp<KT, X2>(best, x, y, x, y, tag);
            traffic_offer_dpp<KT, X3>(best, x, y, x, y, tag);
        }
        if constexpr (W >= 8) {
            const float mx = dpp_f<HALF_MIRROR>(x), my = dpp_f<HALF_MIRROR>(y);
            const int mt = dpp_i<HALF_MIRROR>(tag);
            traffic_offer<KT>(best, x, y, mx, my, mt);            // k ^ 7
            traffic_offer_dpp<KT, X3>(best, x, y, mx, my, mt);    // k ^ 4
            traffic_offer_dpp<KT, X2>(best, x, y, mx, my, mt);    // k ^ 5
            traffic_offer_dpp<KT, X1>(best, x, y, mx, my, mt);    // k ^ 6
        }
    }
}

// features: the record of one kept key — the winner's (x, y, h, vx, vy) fetched by lane index from its group (every lane of the wavefront
// calls this together) and rotated into the observer's frame; `a` words 0..3, `b` words 4..7
template <int W>
__device__ __forceinline__ void traffic_record(uint64_t key, bool active, int lane, const TrafficSelf& me, const TrafficArgs& q, float4& a, float4& b) {
    const bool present = active && key != kTrafficNone;
    const int j = (int)((uint32_t)key & (uint32_t)(W - 1));
    const int src = (lane & ~(W - 1)) + j;
    const float xj = __shfl(me.x, src, 64), yj = __shfl(me.y, src, 64), hj = __shfl(me.h, src, 64);
    const float vxj = __shfl(me.vx, src, 64), vyj = __shfl(me.vy, src, 64);
    const float dx = xj - me.x, dy = yj - me.y;
    const float d = sqrtf(__uint_as_float((uint32_t)(key >> 32)));
    const float ahead = dx * me.sn + dy * me.cs, right = dx * me.cs - dy * me.sn;
    const float dh = hj - me.h;
    const float dvx = vxj - me.vx, dvy = vyj - me.vy;
    const float dva = dvx * me.sn + dvy * me.cs, dvr = dvx * me.cs - dvy * me.sn;
    a = make_float4(1.0f, d * q.s_pos, ahead * q.s_pos, right * q.s_pos);
    b = make_float4(dh / q.h_div, dva * q.s_v, dvr * q.s_v, (float)j);
    if (!present) {
        a = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        b = make_float4(0.0f, 0.0f, 0.0f, -1.0f);
    }
}

template <int W, int KT>
__global__ void __launch_bounds__(kBlock)
k_traffic(int B, int N, atc_state_t st, float* __restrict__ traffic, TrafficArgs q) {
    const int tid = threadIdx.x, lane = tid & 63;
    const uint32_t slot = blockIdx.x * (uint32_t)kBlock + (uint32_t)tid;
    const int k = (int)(slot % W);
    const bool env_valid = slot < (uint32_t)B * (uint32_t)W;
    const int e = env_valid ? (int)(slot / W) : B - 1;   // clamped: loads stay in bounds, nothing is stored
    const bool lane_valid = env_valid && k < N;
    const uint32_t i = lane_valid ? (uint32_t)e * (uint32_t)N + (uint32_t)k : (uint32_t)B * (uint32_t)N - 1u;

    const int4 ps = reinterpret_cast<const int4*>(st.ac)[i];
    const double alt = st.alt[i];
    uint32_t mask = (uint32_t)st.env[(size_t)e * ATC_ENV_WORDS + ATC_ENV_MASK_LO];
    if (W == 64 && k >= 32) mask = (uint32_t)st.stats[(size_t)e * ATC_STAT_WORDS + ATC_STAT_MASK_HI];
    const bool active = lane_valid && ((mask >> (k & 31)) & 1u);

    int phi = ps.z;
    if (is_wide(phi)) phi = phi_wrap(st.phi_wide[4 * (size_t)i]);   // (include/atc_step.h, ABI 19: the exact counts are in the side record)
    const TrafficSelf me = traffic_self(ps.x, ps.y, alt, phi, (uint32_t)ps.w, q);
    const int tag = active ? k : -1;

    // ---- selection ------------------------------------------------------------------------------------------------------
    uint64_t best[KT];
    if constexpr (W >= 32) {
        __shared__ float sx[kBlock], sy[kBlock];
        __shared__ int stag[kBlock];
        sx[tid] = me.x;
        sy[tid] = me.y;
        stag[tid] = tag;
        __syncthreads();
        const int base = tid & ~(W - 1);
        traffic_select<W, KT>(best, me.x, me.y, tag, k, N, sx + base, sy + base, stag + base);
    } else {
        traffic_select<W, KT>(best, me.x, me.y, tag, k, N, nullptr, nullptr, nullptr);
    }

    // ---- features and store -------------------------------------------------------------------------------------------------
    float4* dst = reinterpret_cast<float4*>(traffic + (size_t)i * (size_t)q.K * ATC_TRAFFIC_DIM);
#pragma unroll
    for (int r = 0; r < KT; ++r) {
        float4 a, b;
        traffic_record<W>(best[r], active, lane, me, q, a, b);
        if (lane_valid && r < q.K) {
            if (ATC_TRAFFIC_NT_STORES) {
                typedef float v4f __attribute__((ext_vector_type(4)));
                stream_store(reinterpret_cast<v4f*>(&dst[2 * r]), v4f{a.x, a.y, a.z, a.w});
                stream_store(reinterpret_cast<v4f*>(&dst[2 * r + 1]), v4f{b.x, b.y, b.z, b.w});
            } else {
                dst[2 * r] = a;
                dst[2 * r + 1] = b;
            }
        }
    }
}
