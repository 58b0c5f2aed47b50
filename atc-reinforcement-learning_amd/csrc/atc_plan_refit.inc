// atc_plan_refit.inc — k_plan_refit (atc_plan_refit, include/atc_step.h): the weighted mean and standard deviation of the drawn plans of
// one iteration, with no plan materialised.  Included by atc_step.hip behind atc_plan_sampled.inc, whose plan_cand_key / plan_draw it
// calls: plan_draw stays the one definition of the draw.
//   Flat mapping, k_plan_draw's: one lane per aircraft slot of one segment (blockIdx.y); the lane's mean and std rows are loaded once and
//   the loop over the M candidates runs in registers — candidate m's action block is regenerated, never stored.  Per component the lane
//   accumulates W = sum w, s1 = sum w d and s2 = sum (w d) d with d = a_m - ctr, ctr the clamped mean: the terms scale as std z, so a small
//   std keeps its digits (E[a^2] - E[a]^2 would lose it below about 1e-3).  Every operation is one fp32 rounding (-ffp-contract=off: no
//   product is fused into a sum), sequential in m: tests/plan_refit_ref.py restates it in numpy, bit for bit.
//   A candidate PARTICIPATES in env e iff 0 < weight[m][e] <= FLT_MAX (a NaN fails both comparisons).  A wavefront none of whose lanes'
//   candidates participates skips the draw — three mix64 per component saved: a CEM call costs about E draws per env, not M.  The skip
//   changes no result: a lane whose candidate does not participate adds nothing either way.
//   The division and the square root are the compiler's correctly rounded fp32 forms (the HIP default, -fhip-fp32-correctly-rounded-divide-sqrt;
//   DESIGN.md section 3h).  new_mean / new_std may BE mean / std: a lane reads its 24 bytes before the loop and writes them behind it, and
//   no lane reads another's — hence no __restrict__ on the four.  Every [M][...] and [H][...] offset is a size_t.
struct RefitAcc {
    float s1, s2;
};
__device__ __forceinline__ void refit_add(RefitAcc& acc, float w, float a, float ctr) {
    const float d = a - ctr;
    const float t = w * d;
    acc.s1 = acc.s1 + t;
    acc.s2 = acc.s2 + t * d;
}
__device__ __forceinline__ void refit_close(const RefitAcc& acc, float W, float ctr, float* mean_out, float* std_out) {
    const float q = acc.s1 / W;
    *mean_out = ctr + q;
    *std_out = sqrtf(fmaxf(acc.s2 / W - q * q, 0.0f));
}

__global__ void __launch_bounds__(kBlock)
k_plan_refit(int B, int N, int H, int M, const float* mean, const float* std, atc_plan_draw_t dr, const float* __restrict__ weight,
             float* new_mean, float* new_std) {
    const size_t BN = (size_t)(uint32_t)B * (uint32_t)N;
    const size_t slot = (size_t)blockIdx.x * (uint32_t)kBlock + threadIdx.x;
    const bool valid = slot < BN;                                    // (idle lanes stay for the wave-uniform loop; they load and store nothing)
    const uint32_t i = valid ? (uint32_t)slot : 0u, e = i / (uint32_t)N;   // (B N 40 < 4 GiB: 32-bit byte offsets within a row)
    const uint32_t h = blockIdx.y;
    const size_t row = (size_t)h * BN * 3u;
    Float3 mu = {0.0f, 0.0f, 0.0f}, sd = {0.0f, 0.0f, 0.0f};
    if (valid) {
        mu = *at<Float3>(mean + row, times12(i));
        sd = *at<Float3>(std + row, times12(i));
    }
    const Float3 ctr = {plan_draw_clamp(mu.a), plan_draw_clamp(mu.b), plan_draw_clamp(mu.c)};
    RefitAcc xa = {0.0f, 0.0f}, xb = {0.0f, 0.0f}, xc = {0.0f, 0.0f};
    float W = 0.0f;
    for (uint32_t m = 0; m < (uint32_t)M; ++m) {
        const float w = valid ? weight[(size_t)m * (uint32_t)B + e] : 0.0f;
        const bool part = w > 0.0f && w <= __FLT_MAX__;
        if (__builtin_amdgcn_ballot_w64(part) == 0ull) continue;    // no lane of this wavefront needs candidate m
        const bool mean_only = (dr.flags & ATC_DRAW_MEAN_FIRST) != 0u && m == 0u;
        const Float3 a = plan_draw(plan_cand_key(dr, m), mean_only, h, i, mu, sd);
        if (part) {
            refit_add(xa, w, a.a, ctr.a);
            refit_add(xb, w, a.b, ctr.b);
            refit_add(xc, w, a.c, ctr.c);
            W = W + w;
        }
    }
    if (!valid || !(W > 0.0f)) return;                               // an env with no participating candidate keeps its rows
    Float3 nm, ns;
    refit_close(xa, W, ctr.a, &nm.a, &ns.a);
    refit_close(xb, W, ctr.b, &nm.b, &ns.b);
    refit_close(xc, W, ctr.c, &nm.c, &ns.c);
    *at<Float3>(new_mean + row, times12(i)) = nm;
    *at<Float3>(new_std + row, times12(i)) = ns;
}
