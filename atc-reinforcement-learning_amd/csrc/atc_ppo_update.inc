// atc_ppo_update.inc — what closes a PPO update behind the two gradient calls (include/atc_step.h: atc_adv_normalise, atc_adam_step):
// k_adv_moments and k_adv_apply (mean, std and the normalised advantages of a collection, no host read) and k_adam_step (gradient-norm
// clip, the entropy window and Adam on one or two packed tensors in one launch).  Included by atc_step.hip behind atc_value.inc.
//   FLOAT64 THROUGHOUT, one rounding per stored float32 word, in an order the header spells out: tests/ppo_update_ref.py restates it in
//   numpy and the kernels equal it bit for bit.  The file is built with -ffp-contract=off like every other: a product and the sum behind
//   it are two roundings.  Float64 division and square root are correctly rounded on the device, so their lowering does not enter.
//   DETERMINISM: no atomics.  A lane adds its rows (words) in ascending order, lane 0 folds the lanes' sums from LDS in lane order, and
//   k_adv_apply folds the G partial triples in the order of g — every workgroup does, at wave-uniform addresses.
//   STORES: per-workgroup partials and statistics go out as ordinary vector stores from the lanes that hold them (as in k_ppo_grad).
constexpr int kAdvBlock = ATC_ADV_TILE;          // lanes of a workgroup = rows of a tile
constexpr int kAdvApplyMaxGrid = 2048;           // workgroups of k_adv_apply at most: it strides over the tiles
constexpr int kAdamBlock = ATC_ADAM_BLOCK;

// scratch[g] = {n, S, S2} of the rows of workgroup g's tiles g, g + G, ...: n participating rows, S = sum a, S2 = sum a * a (in float64)
__global__ void __launch_bounds__(kAdvBlock)
k_adv_moments(int R, const float* __restrict__ adv, const uint8_t* __restrict__ mask, double* __restrict__ scratch) {
    __shared__ double fold[3 * kAdvBlock];
    const int lane = threadIdx.x;
    const long long tiles = ((long long)R + (kAdvBlock - 1)) / kAdvBlock;
    double n = 0.0, S = 0.0, S2 = 0.0;
#pragma unroll 4
    for (long long tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
        const long long r = tile * kAdvBlock + lane;
        bool part = r < (long long)R;
        if (part && mask) part = mask[r] != 0;
        const double a = part ? (double)adv[r] : 0.0;        // (a row that takes no part is not read)
        n = part ? n + 1.0 : n;
        S = part ? S + a : S;
        S2 = part ? S2 + a * a : S2;
    }
    fold[lane] = n;
    fold[kAdvBlock + lane] = S;
    fold[2 * kAdvBlock + lane] = S2;
    __syncthreads();
    if (lane == 0) {
        double tn = 0.0, tS = 0.0, tS2 = 0.0;
        for (int l = 0; l < kAdvBlock; ++l) {
            tn += fold[l];
            tS += fold[kAdvBlock + l];
            tS2 += fold[2 * kAdvBlock + l];
        }
        double* const P = scratch + (size_t)blockIdx.x * 3u;
        P[0] = tn;
        P[1] = tS;
        P[2] = tS2;
    }
}

// every workgroup: the G triples in the order of g -> mean, std, shift, scale; then its tiles of rows; workgroup 0 also writes stats.
// adv and out_adv may be the same array (a row is read and written by the same lane), so neither is __restrict__.
__global__ void __launch_bounds__(kAdvBlock)
k_adv_apply(int R, int G, float eps, const float* adv, const uint8_t* __restrict__ mask, const double* __restrict__ scratch, float* out_adv,
            float* __restrict__ stats) {
    double n = 0.0, S = 0.0, S2 = 0.0;
    for (int g = 0; g < G; ++g) {
        n += scratch[(size_t)g * 3u + 0u];
        S += scratch[(size_t)g * 3u + 1u];
        S2 += scratch[(size_t)g * 3u + 2u];
    }
    double mean = 0.0, sd = 0.0;
    float shift = 0.0f, scale = 0.0f;
    if (n > 0.0) {
        mean = S / n;
        double var = 0.0;
        if (n > 1.0) {
            const double c = S2 - S * mean;
            var = (c > 0.0 ? c : 0.0) / (n - 1.0);
        }
        sd = __builtin_sqrt(var);
        shift = (float)mean;
        scale = (float)(1.0 / (sd + (double)eps));
    }
    if (blockIdx.x == 0 && threadIdx.x < ATC_ADV_STATS) {
        const int q = threadIdx.x;
        stats[q] = q == ATC_ADV_STAT_N ? (float)n : q == ATC_ADV_STAT_MEAN ? shift : q == ATC_ADV_STAT_SCALE ? scale : (float)sd;
    }
    if (!out_adv) return;
    const long long tiles = ((long long)R + (kAdvBlock - 1)) / kAdvBlock;
    for (long long tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
        const long long r = tile * kAdvBlock + (long long)threadIdx.x;
        if (r >= (long long)R) break;
        bool part = n > 0.0;
        if (part && mask) part = mask[r] != 0;
        const float a = part ? adv[r] : 0.0f;
        const float z = (a - shift) * scale;
        out_adv[r] = part ? z : 0.0f;                          // a select: what stands in a row that takes no part changes nothing
    }
}

// the kernel's own argument block: the ABI's two structs flattened, the bias corrections made on the host in double
struct AdamTensorArg {
    float* w;
    const float* grad;
    float* m;
    float* v;
    int32_t words;
    float grad_scale;
    int32_t add_first, add_count;
    float add_value;
};
struct AdamArgs {
    AdamTensorArg t[2];          // t[1].words == 0 for a call on one tensor
    double lr, beta1, beta2, eps, max_norm, c1, c2;
    int32_t step;
};

__device__ __forceinline__ double adam_effective_grad(const AdamTensorArg& t, int i) {
    const double add = (i >= t.add_first && i - t.add_first < t.add_count) ? (double)t.add_value : 0.0;
    return (double)t.grad_scale * (double)t.grad[i] + add;
}

// ONE workgroup of 1 024 lanes over the concatenated words j of both tensors: the norm of the effective gradient, then every word's update
__global__ void __launch_bounds__(kAdamBlock)
k_adam_step(AdamArgs a, float* __restrict__ stats) {
    __shared__ double fold[kAdamBlock];
    __shared__ double total_s;
    const int lane = threadIdx.x;
    const int w0 = a.t[0].words, all = w0 + a.t[1].words;
    double s = 0.0;
    for (int j = lane; j < all; j += kAdamBlock) {
        const double ge = j < w0 ? adam_effective_grad(a.t[0], j) : adam_effective_grad(a.t[1], j - w0);
        s += ge * ge;
    }
    fold[lane] = s;
    __syncthreads();
    if (lane == 0) {
        double t = 0.0;
        for (int l = 0; l < kAdamBlock; ++l) t += fold[l];
        total_s = t;
    }
    __syncthreads();
    const double norm = __builtin_sqrt(total_s);
    const bool finite = __builtin_fabs(norm) < __builtin_inf();      // (false for a NaN)
    double coef = 1.0;
    if (a.max_norm > 0.0 && a.max_norm < __builtin_inf()) {
        const double c = a.max_norm / (norm + 1e-6);
        coef = c < 1.0 ? c : 1.0;
    }
    if (lane < ATC_ADAM_STATS)
        stats[lane] = lane == ATC_ADAM_STAT_NORM ? (float)norm : lane == ATC_ADAM_STAT_COEF ? (finite ? (float)coef : 0.0f)
                      : lane == ATC_ADAM_STAT_SKIPPED ? (finite ? 0.0f : 1.0f) : (float)a.step;
    if (!finite) return;                                             // nothing is written to w, m or v
    const double step_size = a.lr / a.c1, root_c2 = __builtin_sqrt(a.c2);
    const double one_b1 = 1.0 - a.beta1, one_b2 = 1.0 - a.beta2;
    for (int j = lane; j < all; j += kAdamBlock) {
        const bool first = j < w0;                                   // (the tensor's pointers by selects: no copy of the block is indexed)
        const int i = first ? j : j - w0;
        float* const w = first ? a.t[0].w : a.t[1].w;
        float* const m = first ? a.t[0].m : a.t[1].m;
        float* const v = first ? a.t[0].v : a.t[1].v;
        const double gc = (first ? adam_effective_grad(a.t[0], i) : adam_effective_grad(a.t[1], i)) * coef;
        const float m32 = (float)(a.beta1 * (double)m[i] + one_b1 * gc);
        const float v32 = (float)(a.beta2 * (double)v[i] + (one_b2 * gc) * gc);
        const double denom = __builtin_sqrt((double)v32) / root_c2 + a.eps;
        m[i] = m32;
        v[i] = v32;
        w[i] = (float)((double)w[i] - step_size * ((double)m32 / denom));
    }
}
