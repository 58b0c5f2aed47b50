// atc_plan_score.inc — k_plan_score (atc_plan_score, include/atc_step.h): the segment rewards of one iteration's M candidates turned into
// a discounted score per candidate, a strict total order per env, the refit weights (elite 0/1 or softmax) and the best R candidate
// numbers, in one launch.  Included by atc_step.hip behind atc_plan_refit.inc.
//   Mapping: ONE LANE PER ENV, workgroups of one wavefront (kScoreBlock = 64).  [M][B] has B contiguous, so row m of seg_reward, n_steps,
//   score and weight is a coalesced access across the wavefront, and a lane only ever touches its own column: no lane reads another
//   env's words, nothing is synchronised, and an idle lane of the last workgroup returns before its first load.
//   Pass 1 (m ascending): the score, operation by operation (-ffp-contract=off: the product and the sum are rounded once each), stored
//   to score[m][e]; the candidate's IMAGE — the order-preserving 32-bit image of the score, -0 mapped to +0's, 0 for an invalid
//   candidate (a finite float's image is >= 0x00800000, so 0 is free) — stored to the weight column, which is the workspace until the
//   last pass overwrites it; the running best (the largest image, the LOWER m on a tie) and the number of valid candidates.
//   ELITE: the image T of the candidate at position E' = min(elites, valid) of the order by a radix select on the image, 4 bits a pass
//   (8 passes over the column), with the lane's 16 counters in LDS (hist[bin][lane]: no two lanes share a word, bank = lane).  The select
//   also leaves `need`, the number of candidates with image == T that belong to the first E'; the last pass runs m ascending and gives
//   1.0f to every image > T and to the first `need` images == T: equal scores go to the lower candidate number.
//   top: row 0 is the running best; row r > 0 is the largest key below row r-1's, key = image << 10 | (M-1-m) (unique per env), one pass
//   of the column each — R <= 64 bounds it, and the passes stop at the first row that finds nothing (-1 from there on).
//   SOFTMAX: one pass, weight = expf((score - smax) / temperature) for a valid candidate, smax the running best's score; the division is
//   the compiler's correctly rounded fp32 form (the HIP default, as in atc_plan_refit.inc).
//   Every [M][...] offset is a size_t.
constexpr int kScoreBlock = 64;

__device__ __forceinline__ uint32_t score_image(float score, bool evaluated) {
    if (!evaluated || !(fabsf(score) <= __FLT_MAX__)) return 0u;      // (a NaN fails the comparison)
    uint32_t u = __float_as_uint(score);
    if (u == 0x80000000u) u = 0u;                                      // -0 orders as +0
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}

__global__ void __launch_bounds__(kScoreBlock)
k_plan_score(int B, int H, int M, const float* __restrict__ seg, const uint16_t* __restrict__ n_steps, atc_plan_score_t sc,
             float* __restrict__ score, float* __restrict__ weight, int32_t* __restrict__ top, int R) {
    __shared__ uint32_t hist[16][kScoreBlock];
    const size_t e = (size_t)blockIdx.x * (uint32_t)kScoreBlock + threadIdx.x;
    if (e >= (size_t)(uint32_t)B) return;                              // idle lanes neither load nor store (nothing below synchronises)
    const size_t Bs = (size_t)(uint32_t)B;
    uint32_t* const image = reinterpret_cast<uint32_t*>(weight);       // the weight column is the workspace until the last pass
    const uint32_t Mu = (uint32_t)M, lane = threadIdx.x;

    // pass 1: score, image, running best, number of valid candidates
    uint32_t best_img = 0u, best_m = 0u, n_valid = 0u;
    float smax = 0.0f;
    for (uint32_t m = 0; m < Mu; ++m) {
        const float* row = seg + (size_t)m * (uint32_t)H * Bs + e;
        float s = row[0], g = 1.0f;
        for (int h = 1; h < H; ++h) {
            g = g * sc.gamma;
            const float t = row[(size_t)h * Bs] * g;
            s = s + t;
        }
        if (s != s) s = __uint_as_float(0x7FC00000u);                  // one NaN: IEEE 754 fixes neither the sign nor the payload of a computed one
        const size_t at_m = (size_t)m * Bs + e;
        const bool evaluated = n_steps == nullptr || n_steps[at_m] != 0;
        const uint32_t img = score_image(s, evaluated);
        score[at_m] = s;
        image[at_m] = img;
        n_valid += img != 0u ? 1u : 0u;
        if (img > best_img) {
            best_img = img;
            best_m = m;
            smax = s;
        }
    }

    // top: row 0 is the running best, every later row the largest key below the row before
    if (R > 0) {
        uint64_t prev = best_img ? ((uint64_t)best_img << 10 | (Mu - 1u - best_m)) : 0ull;
        top[e] = best_img ? (int32_t)best_m : -1;
        for (int r = 1; r < R; ++r) {
            uint64_t found = 0ull;
            if (prev != 0ull && (uint32_t)r < n_valid) {
                for (uint32_t m = 0; m < Mu; ++m) {
                    const uint32_t img = image[(size_t)m * Bs + e];
                    const uint64_t key = (uint64_t)img << 10 | (Mu - 1u - m);
                    if (img != 0u && key < prev && key > found) found = key;
                }
            }
            top[(size_t)r * Bs + e] = found ? (int32_t)(Mu - 1u - (uint32_t)(found & 1023u)) : -1;
            prev = found;
        }
    }

    if (sc.mode == ATC_SCORE_SOFTMAX) {
        for (uint32_t m = 0; m < Mu; ++m) {
            const size_t at_m = (size_t)m * Bs + e;
            float w = 0.0f;
            if (image[at_m] != 0u) {
                const float x = (score[at_m] - smax) / sc.temperature;
                w = expf(x);
            }
            image[at_m] = __float_as_uint(w);       // (one pointer type for the column: workspace and result)
        }
        return;
    }

    // ELITE: radix select of the image at position `need` of the order, four bits a pass, most significant first
    uint32_t need = (uint32_t)sc.elites < n_valid ? (uint32_t)sc.elites : n_valid;
    uint32_t thr = 0u, known = 0u;                                     // thr: the bits found so far; known: the mask of those bits
    if (need != 0u) {
        for (int shift = 28; shift >= 0; shift -= 4) {
            for (int b = 0; b < 16; ++b) hist[b][lane] = 0u;
            for (uint32_t m = 0; m < Mu; ++m) {
                const uint32_t img = image[(size_t)m * Bs + e];
                if (img != 0u && (img & known) == thr) hist[(img >> shift) & 15u][lane] += 1u;
            }
            int b = 15;
            for (; b > 0; --b) {
                const uint32_t c = hist[b][lane];
                if (need <= c) break;
                need -= c;
            }
            thr |= (uint32_t)b << shift;
            known |= 15u << shift;
        }
    }
    // (need is now the number of candidates with image == thr among the first min(elites, valid) of the order: the lowest m take them)
    for (uint32_t m = 0; m < Mu; ++m) {
        const size_t at_m = (size_t)m * Bs + e;
        const uint32_t img = image[at_m];
        float w = 0.0f;
        if (img != 0u && thr != 0u) {
            if (img > thr) w = 1.0f;
            else if (img == thr && need != 0u) {
                w = 1.0f;
                --need;
            }
        }
        image[at_m] = __float_as_uint(w);       // (one pointer type for the column: workspace and result)
    }
}
