// atc_abi.inc — the C-ABI entry points of libatcstep.so (include/atc_step.h): argument checks, scenario upload, the launches of the
// query / reset / observe kernels, atc_step and its relatives, the host side of the result-packet polling and of the persistent step
// server.  Included at the end of atc_step.hip (one translation unit: the entry points instantiate the kernel templates through
// step_common / launch_step); nothing here runs on the device.
extern "C" {

int atc_abi_version(void) { return ATC_ABI_VERSION; }

// every launch record's getter: the first min(n, slots) counters of the calling thread
static int copy_counts(Record rec, uint64_t* out, int n) {
    if (!out || n < 0) return fail_arg("null pointer");
    for (int i = 0; i < n && i < kRecordSlots[rec]; ++i) out[i] = record(rec)[i];
    return ATC_OK;
}
int atc_launch_counts(uint64_t* out, int n) { return copy_counts(REC_STEP, out, n); }
int atc_skip_launch_counts(uint64_t* out, int n) { return copy_counts(REC_SKIP, out, n); }
int atc_traffic_launch_counts(uint64_t* out, int n) { return copy_counts(REC_TRAFFIC, out, n); }
int atc_lookahead_launch_counts(uint64_t* out, int n) { return copy_counts(REC_LOOKAHEAD, out, n); }
int atc_plan_launch_counts(uint64_t* out, int n) { return copy_counts(REC_PLAN, out, n); }
int atc_plan_sampled_launch_counts(uint64_t* out, int n) { return copy_counts(REC_PLAN_SAMPLED, out, n); }
int atc_plan_draw_launch_counts(uint64_t* out, int n) { return copy_counts(REC_PLAN_DRAW, out, n); }
int atc_plan_refit_launch_counts(uint64_t* out, int n) { return copy_counts(REC_PLAN_REFIT, out, n); }
int atc_plan_score_launch_counts(uint64_t* out, int n) { return copy_counts(REC_PLAN_SCORE, out, n); }
int atc_branch_launch_counts(uint64_t* out, int n) { return copy_counts(REC_BRANCH, out, n); }
int atc_select_launch_counts(uint64_t* out, int n) { return copy_counts(REC_SELECT, out, n); }
int atc_rollout_policy_launch_counts(uint64_t* out, int n) { return copy_counts(REC_POLICY, out, n); }
int atc_rollout_policy_traffic_launch_counts(uint64_t* out, int n) { return copy_counts(REC_POLICY_TRAFFIC, out, n); }
int atc_gae_launch_counts(uint64_t* out, int n) { return copy_counts(REC_GAE, out, n); }
int atc_rollout_policy_ends_launch_counts(uint64_t* out, int n) { return copy_counts(REC_POLICY_ENDS, out, n); }
int atc_gae_boot_launch_counts(uint64_t* out, int n) { return copy_counts(REC_GAE_BOOT, out, n); }
int atc_ppo_policy_grad_launch_counts(uint64_t* out, int n) { return copy_counts(REC_PPO_GRAD, out, n); }
int atc_value_forward_launch_counts(uint64_t* out, int n) { return copy_counts(REC_VALUE_FORWARD, out, n); }
int atc_ppo_value_grad_launch_counts(uint64_t* out, int n) { return copy_counts(REC_PPO_VALUE_GRAD, out, n); }
int atc_policy_eval_launch_counts(uint64_t* out, int n) { return copy_counts(REC_POLICY_EVAL, out, n); }
int atc_adv_normalise_launch_counts(uint64_t* out, int n) { return copy_counts(REC_ADV_NORMALISE, out, n); }
int atc_adam_step_launch_counts(uint64_t* out, int n) { return copy_counts(REC_ADAM_STEP, out, n); }
int atc_policy_forward_launch_counts(uint64_t* out, int n) { return copy_counts(REC_POLICY_FORWARD, out, n); }
int atc_lookahead_policy_launch_counts(uint64_t* out, int n) { return copy_counts(REC_LOOKAHEAD_POLICY, out, n); }
int atc_rollout_policy_term_launch_counts(uint64_t* out, int n) { return copy_counts(REC_POLICY_TERM, out, n); }
int atc_lookahead_set_mapping(int candidates_per_workgroup) {
    if (candidates_per_workgroup < 0 || candidates_per_workgroup > ATC_LOOKAHEAD_MAX_M) return fail_arg("candidates per workgroup must be 0 (the library's choice) .. 64");
    t_look_cpg = candidates_per_workgroup;
    return ATC_OK;
}
int atc_fill_prefetch_info(const atc_scenario_t* s, int B, int N, int* resident, int* stride) {
    if (!s || !resident || !stride) return fail_arg("null pointer");
    if (B < 1 || N < 1 || N > ATC_MAX_AIRCRAFT) return fail_arg("need B >= 1, 1 <= N <= 64");
    *resident = *stride = 0;
    return with_width(N, [&](auto w) {
        constexpr int W = decltype(w)::value;
        if constexpr (W <= 16) {
            if (N != W || ((long long)B * W) % kBlock != 0) return ATC_OK;   // (not the all-valid form: no prefetch)
            if (const int rc = fill_prefetch_resident<W>(s, resident)) return rc;
            if (fill_prefetch_enabled() && step_grid(B, W) > *resident) *stride = *resident;
        }
        return ATC_OK;
    });
}
const char* atc_last_error(void) { return g_err; }

int atc_host_mapped_ptr(const void* host, void** dev) {
    if (!host || !dev) return fail_arg("null pointer");
    HIP_TRY(hipHostGetDevicePointer(dev, const_cast<void*>(host), 0));
    return 0;
}

int atc_scenario_create(const float* blob_host, size_t n_words, int device, atc_scenario_t** out) {
    if (!blob_host || !out) return fail_arg("null pointer");
    if (n_words < ATC_C_END || blob_host[ATC_H_VERSION] != ATC_BLOB_VERSION || (size_t)blob_host[ATC_H_NWORDS] != n_words)
        return fail_arg("not a scenario blob of this ABI version");
    if ((int)blob_host[ATC_H_N_MVA] > 32) return fail_arg("at most 32 MVA polygons");
    if ((int)blob_host[ATC_H_N_ENTRY] > 0) {   // the spawn records every reset reads
        const size_t os = (size_t)blob_host[ATC_H_OFF_SPAWN];
        if (os == 0 || os % 16 != 0 || os + (size_t)(ATC_MAX_AIRCRAFT + (int)blob_host[ATC_H_N_ENTRY]) * ATC_SPAWN_WORDS > n_words)
            return fail_arg("spawn records (ATC_H_OFF_SPAWN) missing, misaligned or beyond the blob");
    }
    if ((int)blob_host[ATC_H_N_NOISE] > 16) return fail_arg("at most 16 noise-abatement areas");
    if (const int og = (int)blob_host[ATC_H_OFF_GRID]) {   // the kernel clamps cell indices into the grid's outermost ring
        if ((size_t)og + ATC_G_HDR > n_words) return fail_arg("lookup grid offset beyond the blob");
        const float* g = blob_host + og;
        const long nx = (long)g[ATC_G_NX], ny = (long)g[ATC_G_NY];
        if (nx < 3 || ny < 3 || nx >= (1 << 20) || ny >= (1 << 20) || (size_t)og + ATC_G_HDR + 2 * (size_t)nx * ny > n_words)
            return fail_arg("lookup grid dimensions");
        const float* c = g + ATC_G_HDR;
        for (long i = 0; i < nx; ++i)
            if (c[2 * i] != 0.0f || c[2 * i + 1] != 0.0f || c[2 * ((ny - 1) * nx + i)] != 0.0f || c[2 * ((ny - 1) * nx + i) + 1] != 0.0f)
                return fail_arg("the outermost ring of lookup cells must be clean and outside the airspace");
        for (long j = 0; j < ny; ++j)
            if (c[2 * j * nx] != 0.0f || c[2 * j * nx + 1] != 0.0f || c[2 * (j * nx + nx - 1)] != 0.0f || c[2 * (j * nx + nx - 1) + 1] != 0.0f)
                return fail_arg("the outermost ring of lookup cells must be clean and outside the airspace");
    }
    {   // compiled-in aircraft constants (csrc/atc_device.h) must match the blob
        const float want[] = {kVMin, kVMax, kHMin, kHMax, kAMin, kAMax, kHDotMin, kHDotMax, kPhiDotMin, kPhiDotMax, kVInit};
        for (int c = 0; c < 11; ++c)
            if (blob_host[ATC_C_V_MIN + c] != want[c]) return fail_arg("aircraft limits differ from the compiled-in constants");
        if (blob_host[ATC_C_ACT_DISCR] != kDiscrV || blob_host[ATC_C_ACT_DISCR + 1] != kDiscrH ||
            blob_host[ATC_C_ACT_DISCR + 2] != kDiscrPhi)
            return fail_arg("action discriminator differs from the compiled-in constants");
    }
    HIP_TRY(hipSetDevice(device));
    static std::atomic<uint64_t> next_uid{1};
    atc_scenario* s = new atc_scenario();
    s->uid = next_uid.fetch_add(1);
    s->n_words = (int)n_words;
    s->off_grid = (int)blob_host[ATC_H_OFF_GRID];
    memcpy(s->consts, blob_host, sizeof s->consts);
    memset(s->ghdr, 0, sizeof s->ghdr);
    if (s->off_grid) memcpy(s->ghdr, blob_host + s->off_grid, sizeof s->ghdr);
    s->device = device;
    hipDeviceProp_t prop;
    hipError_t e = hipGetDeviceProperties(&prop, device);
    if (e != hipSuccess) {
        delete s;
        return fail_hip(e, "hipGetDeviceProperties");
    }
    s->n_cu = prop.multiProcessorCount > 0 ? prop.multiProcessorCount : 256;
    s->d_lds = nullptr;
    memset(&s->lt, 0, sizeof s->lt);
    s->lds_tab_bytes = 0;
    s->max_lds = (int)prop.sharedMemPerBlock;
    {   // gfx950: 160 KB of LDS per CU, all of it available to one workgroup that opts in (hipFuncAttributeMaxDynamicSharedMemorySize)
        int optin = 0;
        if (hipDeviceGetAttribute(&optin, hipDeviceAttributeSharedMemPerBlockOptin, device) == hipSuccess && optin > s->max_lds) s->max_lds = optin;
        (void)hipGetLastError();
    }
    s->cu_lds = (int)std::max<size_t>(prop.maxSharedMemoryPerMultiProcessor, (size_t)s->max_lds);
    e = hipMalloc(&s->d_blob, n_words * sizeof(float));
    if (e != hipSuccess) {
        delete s;
        return fail_hip(e, "hipMalloc");
    }
    e = hipMemcpy(s->d_blob, blob_host, n_words * sizeof(float), hipMemcpyHostToDevice);
    if (e != hipSuccess) {
        (void)hipFree(s->d_blob);
        delete s;
        return fail_hip(e, "hipMemcpy");
    }
    *out = s;
    return ATC_OK;
}

int atc_scenario_destroy(atc_scenario_t* s) {
    if (!s) return ATC_OK;
    (void)hipFree(s->d_blob);
    if (s->d_lds) (void)hipFree(s->d_lds);
    delete s;
    return ATC_OK;
}

// The LDS-resident lookup table (include/atc_step.h; format: atc_hip/scenario.py:build_lds_table).  Every index the kernel will follow
// is checked HERE, once: codes are trusted on the device (an out-of-range payload would read LDS beyond the table).
int atc_scenario_attach_lds_table(atc_scenario_t* s, const void* table_host, size_t n_bytes) {
    if (!s) return fail_arg("null pointer");
    if (!table_host || n_bytes == 0) {   // detach
        if (s->d_lds) (void)hipFree(s->d_lds);
        s->d_lds = nullptr;
        memset(&s->lt, 0, sizeof s->lt);
        s->lds_tab_bytes = 0;
        return ATC_OK;
    }
    if (!s->off_grid) return fail_arg("the LDS table needs the sector's lookup grid behind it (points it cannot answer go there)");
    if ((int)s->consts[ATC_H_N_NOISE] != 0) return fail_arg("the LDS table does not carry noise-abatement candidates: sectors without such areas only");
    if (n_bytes < 4 * ATC_LDS_HDR_WORDS || n_bytes % 16 != 0) return fail_arg("LDS table: size");
    const uint32_t* h = static_cast<const uint32_t*>(table_host);
    if (h[ATC_LDS_H_MAGIC] != ATC_LDS_MAGIC || h[ATC_LDS_H_BYTES] != n_bytes) return fail_arg("not an LDS lookup table of this ABI version");
    const size_t nx = h[ATC_LDS_H_NX], ny = h[ATC_LDS_H_NY], off_l1 = h[ATC_LDS_H_OFF_L1], off_sub = h[ATC_LDS_H_OFF_SUB], n_sub = h[ATC_LDS_H_N_SUB],
                 off_line = h[ATC_LDS_H_OFF_LINE], n_line = h[ATC_LDS_H_N_LINE], off_hts = h[ATC_LDS_H_OFF_HTS], off_resid = h[ATC_LDS_H_OFF_RESID],
                 n_resid = h[ATC_LDS_H_N_RESID], lds_part = h[ATC_LDS_H_LDS_BYTES], off_pool = h[ATC_LDS_H_OFF_POOL], n_rec = h[ATC_LDS_H_N_REC];
    if (h[ATC_LDS_H_SUB] != 8 || nx < 3 || ny < 3 || nx >= (1u << 11) || ny >= (1u << 11) || n_sub >= (1u << 13) || n_line < 1 || n_line >= (1u << 13) ||
        n_resid >= (1u << 13) || n_rec >= (1u << 24))
        return fail_arg("LDS table: dimensions");
    if (off_l1 != 4 * ATC_LDS_HDR_WORDS || off_sub % 16 || off_line % 16 || off_hts % 16 || off_resid % 4 || lds_part % 16 || off_pool % 16 ||
        off_l1 + 2 * nx * ny > off_sub || off_sub + 2 * 64 * n_sub > off_line || off_line + 32 * n_line > off_hts || off_hts + 4 * 64 > off_resid ||
        off_resid + 4 * n_resid > lds_part || lds_part > off_pool || off_pool + 32 * n_rec > n_bytes)
        return fail_arg("LDS table: section offsets");
    const char* base = static_cast<const char*>(table_host);
    const uint16_t* l1 = reinterpret_cast<const uint16_t*>(base + off_l1);
    const uint16_t* l2 = reinterpret_cast<const uint16_t*>(base + off_sub);
    const uint32_t* ww = reinterpret_cast<const uint32_t*>(base + off_resid);
    auto code_ok = [&](uint16_t c, bool level1) {
        const unsigned kind = (c >> 13) & 3u, pay = c & 0x1fffu;
        if (!level1 && (c & 0x8000u)) return false;
        if (kind == ATC_LDS_CLEAN) return pay <= 63u;
        if (kind == ATC_LDS_LINE) return pay < n_line;
        if (kind == ATC_LDS_SUB) return level1 && pay < n_sub;
        return !level1 && pay < n_resid;   // RESIDUAL: sub-cells only (a level-1 cell that is neither clean nor split is refined)
    };
    for (size_t i = 0; i < nx * ny; ++i)
        if (!code_ok(l1[i], true)) return fail_arg("LDS table: level-1 code");
    for (size_t i = 0; i < 64 * n_sub; ++i)
        if (!code_ok(l2[i], false)) return fail_arg("LDS table: sub-cell code");
    for (size_t i = 0; i < n_resid; ++i) {
        const size_t first = ww[i] & 0xffffffu, n = ww[i] >> 24;
        if (n < 1 || n >= 64 || first + n > n_rec) return fail_arg("LDS table: walk word");
    }
    for (size_t i = 0; i < nx; ++i)
        if (l1[i] || l1[(ny - 1) * nx + i]) return fail_arg("LDS table: the outermost ring of level-1 cells must be clean and outside the airspace");
    for (size_t j = 0; j < ny; ++j)
        if (l1[j * nx] || l1[j * nx + nx - 1]) return fail_arg("LDS table: the outermost ring of level-1 cells must be clean and outside the airspace");
    if (lds_bytes(s, false, true) + lds_part > (size_t)s->max_lds) return fail_arg("LDS table: larger than the device's LDS per workgroup");
    HIP_TRY(hipSetDevice(s->device));
    void* d = nullptr;
    HIP_TRY(hipMalloc(&d, n_bytes));
    hipError_t e = hipMemcpy(d, table_host, n_bytes, hipMemcpyHostToDevice);
    if (e != hipSuccess) {
        (void)hipFree(d);
        return fail_hip(e, "hipMemcpy");
    }
    if (s->d_lds) (void)hipFree(s->d_lds);
    s->d_lds = d;
    s->lds_tab_bytes = lds_part;
    float f[3];
    memcpy(f, h + ATC_LDS_H_X0, sizeof f);
    s->lt = LdsTab{static_cast<const uint4*>(d), (int)(lds_part / 16), f[0], f[1], f[2], (int)nx, (int)nx - 1, (int)ny - 1,
                   (int)off_l1, (int)off_sub, (int)off_line, (int)off_hts, (int)off_resid, static_cast<const char*>(d) + off_pool};
    return ATC_OK;
}

int atc_query_mva_lds(const atc_scenario_t* s, int n, const float* x, const float* y, int32_t* out_h, uint8_t* from_lds, void* stream) {
    if (!s || !x || !y || !out_h || n < 0) return fail_arg("null pointer / negative n");
    if (!s->lt.src) return fail_arg("no LDS lookup table attached");
    if (n == 0) return ATC_OK;
    static thread_local int raised_for = -1;
    if (raised_for != s->device) {
        HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void*>(&k_query_mva_lds), hipFuncAttributeMaxDynamicSharedMemorySize, s->max_lds));
        raised_for = s->device;
    }
    const int blocks = (int)std::min<long long>(((long long)n + kBlock - 1) / kBlock, (long long)s->n_cu);
    hipLaunchKernelGGL(k_query_mva_lds, dim3(blocks), dim3(kBlock), s->lds_tab_bytes, (hipStream_t)stream, s->d_blob, s->off_grid, s->lt, n, x, y,
                       out_h, from_lds);
    HIP_TRY(hipGetLastError());
    return ATC_OK;
}

int atc_query_mva(const atc_scenario_t* s, int n, const float* x, const float* y, int32_t* out_h, int use_grid,
                  void* stream) {
    if (!s || !x || !y || !out_h || n < 0) return fail_arg("null pointer / negative n");
    if (n == 0) return ATC_OK;
    hipLaunchKernelGGL(k_query_mva, dim3(grid_for(s, n)), dim3(kBlock), lds_bytes(s, false), (hipStream_t)stream,
                       s->d_blob, use_grid ? s->off_grid : 0, n, x, y, out_h, (int32_t*)nullptr);
    HIP_TRY(hipGetLastError());
    return ATC_OK;
}
// index variant used by the host mirror's Airspace.find_mva (returns the polygon index, -1 outside)
int atc_query_mva_index(const atc_scenario_t* s, int n, const float* x, const float* y, int32_t* out_idx, int use_grid,
                        void* stream) {
    if (!s || !x || !y || !out_idx || n < 0) return fail_arg("null pointer / negative n");
    if (n == 0) return ATC_OK;
    hipLaunchKernelGGL(k_query_mva, dim3(grid_for(s, n)), dim3(kBlock), lds_bytes(s, false), (hipStream_t)stream,
                       s->d_blob, use_grid ? s->off_grid : 0, n, x, y, (int32_t*)nullptr, out_idx);
    HIP_TRY(hipGetLastError());
    return ATC_OK;
}

int atc_query_corridor(const atc_scenario_t* s, int n, const float* x, const float* y, const float* h, const float* phi,
                       int angle_only, uint8_t* out, void* stream) {
    if (!s || !x || !y || !h || !phi || !out || n < 0) return fail_arg("null pointer / negative n");
    if (n == 0) return ATC_OK;
    hipLaunchKernelGGL(k_query_corridor, dim3(grid_for(s, n)), dim3(kBlock), lds_bytes(s, false), (hipStream_t)stream,
                       s->d_blob, n, x, y, h, phi, angle_only, out);
    HIP_TRY(hipGetLastError());
    return ATC_OK;
}

int atc_query_shaping(const atc_scenario_t* s, int n, const float* d_faf, const float* phi_rel_faf, const float* phi_plane,
                      const float* h, const float* on_gp, float* out3, void* stream) {
    if (!s || !d_faf || !phi_rel_faf || !phi_plane || !h || !on_gp || !out3 || n < 0)
        return fail_arg("null pointer / negative n");
    if (n == 0) return ATC_OK;
    hipLaunchKernelGGL(k_query_shaping, dim3(grid_for(s, n)), dim3(kBlock), lds_bytes(s, false), (hipStream_t)stream,
                       s->d_blob, n, d_faf, phi_rel_faf, phi_plane, h, on_gp, out3);
    HIP_TRY(hipGetLastError());
    return ATC_OK;
}

int atc_reset(const atc_scenario_t* s, int B, int N, const atc_state_t* st, const uint8_t* mask, float* obs,
              const atc_params_t* p, int first, void* stream) {
    if (const int rc = check_env_args(s, B, N, st, p)) return rc;
    hipStream_t q = (hipStream_t)stream;
    hipLaunchKernelGGL(k_reset, dim3(grid_for(s, (long long)B * N)), dim3(kBlock), lds_bytes(s, false), q, s->d_blob,
                       B, N, *st, mask, obs, *p, first);
    HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(k_reset_env, dim3((B + kBlock - 1) / kBlock), dim3(kBlock), 0, q, B, N, *st, mask, first);
    HIP_TRY(hipGetLastError());
    return ATC_OK;
}

int atc_observe(const atc_scenario_t* s, int B, int N, const atc_state_t* st, const uint8_t* mask, float* obs,
                const atc_params_t* p, void* stream) {
    if (!obs) return fail_arg("null pointer");
    if (const int rc = check_env_args(s, B, N, st, p)) return rc;
    hipLaunchKernelGGL(k_observe, dim3(grid_for(s, (long long)B * N)), dim3(kBlock), lds_bytes(s, false),
                       (hipStream_t)stream, s->d_blob, B, N, *st, mask, obs);
    HIP_TRY(hipGetLastError());
    return ATC_OK;
}

int atc_step(const atc_scenario_t* s, int B, int N, const atc_state_t* st, const float* actions, const atc_out_t* out,
             const atc_params_t* p, void* stream) {
    return step_common(s, B, N, 1, 1, st, actions, out, p, stream);
}

int atc_step_packet(const atc_scenario_t* s, const atc_state_t* st, const float* actions, const atc_out_t* out,
                    atc_params_t* p, uint32_t seq, const uint32_t* packet_host, uint32_t* payload, int timeout_us, void* stream) {
    if (!p || !out || !out->packet || !packet_host || !payload) return fail_arg("atc_step_packet needs out->packet, packet_host, payload");
    if (!actions) return fail_arg("null pointer");
    if (reinterpret_cast<uintptr_t>(packet_host) & 15u) return fail_arg("packet_host must be 16-byte aligned");
    p->reserved0 = seq;
    t_inline_action = actions;   // HOST pointer to the 3 action values: they travel in the kernel arguments
    const int rc = step_common(s, 1, 1, 1, 1, st, actions, out, p, stream);
    t_inline_action = nullptr;
    if (rc != ATC_OK) return rc;
    // Every chunk is ONE 16-byte device store and is read here with ONE aligned 16-byte load (movdqa: a single access on every
    // x86-64 with AVX — the tag and the payload words it validates come from the same access, so a reader can never pair a
    // current tag with a stale payload word, whatever order the chunks or the words of other chunks become visible in).
    const auto t0 = std::chrono::steady_clock::now();
    unsigned have = 0;   // bit c: chunk c taken
    for (unsigned it = 1;; ++it) {
        for (int c = 0; c < ATC_PKT_CHUNKS; ++c) {
            if (have >> c & 1u) continue;
            const __m128i v = _mm_load_si128(reinterpret_cast<const __m128i*>(packet_host + 4 * c));
            alignas(16) uint32_t w[4];
            _mm_store_si128(reinterpret_cast<__m128i*>(w), v);
            if (w[3] == seq) {
                payload[3 * c] = w[0];
                payload[3 * c + 1] = w[1];
                payload[3 * c + 2] = w[2];
                have |= 1u << c;
            }
        }
        if (have == (1u << ATC_PKT_CHUNKS) - 1u) return ATC_OK;
        asm volatile("" ::: "memory");   // the buffer changes under us: reload on the next round
        // The result arrives ~10 us after the launch: spin with the pipeline hint first, then give the core away between
        // polls (eight SubprocVecEnv-style workers no longer pin eight cores while they wait).
        if (it < 4096u) _mm_pause();
        else sched_yield();
        if ((it & 255u) == 0 &&
            std::chrono::duration_cast<std::chrono::microseconds>(std::chrono::steady_clock::now() - t0).count() > timeout_us)
            return -3;
    }
}

// ---- persistent step server (include/atc_step.h: atc_serve_*) ------------------------------------------------------------
int atc_serve_start(const atc_scenario_t* s, const atc_state_t* st, const atc_out_t* out, const atc_params_t* p,
                    uint32_t* mailbox_host, uint32_t seq, int lease_us, void* stream) {
    if (!out || !mailbox_host) return fail_arg("null pointer");
    if (const int rc = check_env_args(s, 1, 1, st, p)) return rc;
    if (!out->obs || !out->reward || !out->done || !out->flags || !out->packet) return fail_arg("the server needs obs/reward/done/flags and out->packet");
    if (reinterpret_cast<uintptr_t>(mailbox_host) & 63u) return fail_arg("mailbox must be 64-byte aligned");
    if (!(p->dt > 0.0) || !(0.1423 * p->dt * (double)s->consts[ATC_C_POS_SCALE] < 1073741824.0) || !((double)kAMax * p->dt < 255.9))
        return fail_arg("dt out of range for the fixed-point state formats (see include/atc_step.h)");
    if (lease_us < 10) lease_us = 10;
    uint32_t* mb_dev = nullptr;
    HIP_TRY(hipHostGetDevicePointer(reinterpret_cast<void**>(&mb_dev), mailbox_host, 0));
    // the command word holds the LAST served sequence number (so a stale command is not taken for a new one), no state yet
    __atomic_store_n(mailbox_host + ATC_MB_SEQ, seq, __ATOMIC_RELAXED);
    __atomic_store_n(mailbox_host + ATC_MB_STATE, (uint32_t)ATC_SERVE_IDLE, __ATOMIC_RELEASE);
    hipLaunchKernelGGL(k_serve, dim3(1), dim3(64), lds_bytes(s, false, true), (hipStream_t)stream, s->d_blob, s->off_grid, *st, *out, *p,
                       derive(*p, s, 0), mb_dev, seq, (unsigned long long)lease_us * 100ull);
    HIP_TRY(hipGetLastError());
    ++record(REC_STEP)[ATC_LAUNCH_SERVE];
    return ATC_OK;
}

int atc_serve_step(uint32_t* mailbox_host, const float* actions, uint32_t seq, const uint32_t* packet_host, uint32_t* payload, int timeout_us) {
    if (!mailbox_host || !actions || !packet_host || !payload) return fail_arg("null pointer");
    if (seq == ATC_SERVE_QUIT) return fail_arg("sequence number reserved for the quit command");
    {   // {action, seq} as ONE 16-byte store: the server can never pair a new sequence number with an old action word
        alignas(16) uint32_t w[4];
        memcpy(w, actions, 12);
        w[3] = seq;
        _mm_store_si128(reinterpret_cast<__m128i*>(mailbox_host + ATC_MB_CMD), _mm_load_si128(reinterpret_cast<const __m128i*>(w)));
    }
    const auto t0 = std::chrono::steady_clock::now();
    unsigned have = 0;
    bool left_seen = false;
    for (unsigned it = 1;; ++it) {
        for (int c = 0; c < ATC_PKT_CHUNKS; ++c) {
            if (have >> c & 1u) continue;
            alignas(16) uint32_t w[4];
            _mm_store_si128(reinterpret_cast<__m128i*>(w), _mm_load_si128(reinterpret_cast<const __m128i*>(packet_host + 4 * c)));
            if (w[3] == seq) {
                payload[3 * c] = w[0];
                payload[3 * c + 1] = w[1];
                payload[3 * c + 2] = w[2];
                have |= 1u << c;
            }
        }
        if (have == (1u << ATC_PKT_CHUNKS) - 1u) return ATC_OK;
        if (left_seen) return -4;   // the server had left before it saw this command (lease): the caller starts it again
        asm volatile("" ::: "memory");
        if (it < 4096u) _mm_pause();
        else sched_yield();
        if ((it & 63u) == 0) {
            // (checked once more against the packet above before giving up: a step completed just before the lease ran out counts)
            if (have == 0 && __atomic_load_n(mailbox_host + ATC_MB_STATE, __ATOMIC_ACQUIRE) >= (uint32_t)ATC_SERVE_LEFT_LEASE) left_seen = true;
            if ((it & 255u) == 0 &&
                std::chrono::duration_cast<std::chrono::microseconds>(std::chrono::steady_clock::now() - t0).count() > timeout_us)
                return -3;
        }
    }
}

int atc_serve_stop(uint32_t* mailbox_host, void* stream) {
    if (!mailbox_host) return fail_arg("null pointer");
    __atomic_store_n(mailbox_host + ATC_MB_SEQ, ATC_SERVE_QUIT, __ATOMIC_RELEASE);
    HIP_TRY(hipStreamSynchronize((hipStream_t)stream));   // the state is in memory again once the kernel has ended
    return ATC_OK;
}

int atc_step_multi(int n, const atc_step_call_t* calls) {
    if (n < 0 || (n > 0 && !calls)) return fail_arg("null pointer");
    for (int i = 0; i < n; ++i) {
        const atc_step_call_t& c = calls[i];
        const int rc = step_common(c.s, c.B, c.N, 1, 1, c.st, c.actions, c.out, c.p, c.stream);
        if (rc != ATC_OK) return rc;
    }
    return ATC_OK;
}

int atc_rollout(const atc_scenario_t* s, int B, int N, int T, const atc_state_t* st, const float* actions,
                const atc_out_t* out, const atc_params_t* p, void* stream) {
    return step_common(s, B, N, T, 1, st, actions, out, p, stream);
}

int atc_rollout_hold(const atc_scenario_t* s, int B, int N, int T, int hold, const atc_state_t* st, const float* actions,
                     const atc_out_t* out, const atc_params_t* p, void* stream) {
    return step_common(s, B, N, T, hold, st, actions, out, p, stream);
}

int atc_step_skip(const atc_scenario_t* s, int B, int N, int K, const atc_state_t* st, const float* actions, const atc_out_t* out,
                  uint8_t* n_steps, const atc_params_t* p, void* stream) {
    // K first, before any pointer is looked at
    if (K < 1 || K > ATC_SKIP_MAX) return fail_arg("K (the frame-skip length) must be 1 .. 255");
    if (!actions || !out) return fail_arg("null pointer");
    if (const int rc = check_env_args(s, B, N, st, p)) return rc;
    if (const int rc = check_required_outputs(out)) return rc;
    if (out->packet) return fail_arg("atc_out_t.packet must be NULL for atc_step_skip (the packet is a single step's result)");
    if (p->mode & ATC_M_ACTIONS_HELD) return fail_arg("ATC_M_ACTIONS_HELD is for atc_step only: a frame-skip call's first step carries a fresh decision");
    if (const int rc = check_dt(s, p)) return rc;
    return with_width(N, [&](auto w) { return launch_skip<decltype(w)::value>(s, B, N, K, st, actions, out, n_steps, p, (hipStream_t)stream); });
}

int atc_observe_traffic(const atc_scenario_t* s, int B, int N, int K, const atc_state_t* st, float* traffic, const atc_params_t* p,
                        void* stream) {
    // K first, before any pointer is looked at
    if (K < 1 || K > ATC_TRAFFIC_MAX_K) return fail_arg("K (traffic records per aircraft) must be 1 .. 8");
    if (!traffic) return fail_arg("null pointer");
    if (const int rc = check_env_args(s, B, N, st, p)) return rc;
    const TrafficArgs q = traffic_common(s, p, K);
    return with_width(N, [&](auto w) { return launch_traffic<decltype(w)::value>(B, N, st, traffic, q, (hipStream_t)stream); });
}

int atc_lookahead(const atc_scenario_t* s, int B, int N, int K, int M, const atc_state_t* st, const float* actions,
                  const atc_lookahead_out_t* out, const atc_params_t* p, void* stream) {
    if (const int rc = check_candidates(s, B, N, K, nullptr, M, st, actions, out, p, "look-ahead", "atc_lookahead_out_t", "candidate")) return rc;
    return launch_candidates(REC_LOOKAHEAD, s, B, N, M, out, cand_any(out), p, [&](auto w, auto full, const CandGrid& g, size_t lds, const atc_out_t& o, const StepDerived& q) {
        hipLaunchKernelGGL((k_lookahead<decltype(w)::value, decltype(full)::value>), dim3(g.grid), dim3(kBlock), lds, (hipStream_t)stream, s->d_blob, s->off_grid, B, N, K, M, *st, actions, o, *p, q, out->n_steps, g.cpg, g.groups, g.tiles);
    });
}

int atc_lookahead_plan(const atc_scenario_t* s, int B, int N, int K, int H, int M, const atc_state_t* st, const float* actions,
                       const atc_plan_out_t* out, const atc_params_t* p, void* stream) {
    if (const int rc = check_candidates(s, B, N, K, &H, M, st, actions, out, p, "segment", "atc_plan_out_t", "segment")) return rc;
    return launch_candidates(REC_PLAN, s, B, N, M, out, cand_any(out), p, [&](auto w, auto full, const CandGrid& g, size_t lds, const atc_out_t& o, const StepDerived& q) {
        hipLaunchKernelGGL((k_plan<decltype(w)::value, decltype(full)::value>), dim3(g.grid), dim3(kBlock), lds, (hipStream_t)stream, s->d_blob, s->off_grid, B, N, K, H, M, *st, actions, o, *p, q, out->n_steps, out->seg_reward, g.cpg, g.groups, g.tiles);
    });
}

int atc_lookahead_plan_sampled(const atc_scenario_t* s, int B, int N, int K, int H, int M, const atc_state_t* st, const float* mean,
                               const float* std, const atc_plan_draw_t* dr, const atc_plan_out_t* out, const atc_params_t* p, void* stream) {
    if (const int rc = check_candidates(s, B, N, K, &H, M, st, nullptr, out, p, "segment", "atc_plan_out_t", "segment", {need_dr(dr), need_mean(mean), need_std(std)}))
        return rc;
    return launch_candidates(REC_PLAN_SAMPLED, s, B, N, M, out, cand_any(out), p, [&](auto w, auto full, const CandGrid& g, size_t lds, const atc_out_t& o, const StepDerived& q) {
        hipLaunchKernelGGL((k_plan_sampled<decltype(w)::value, decltype(full)::value>), dim3(g.grid), dim3(kBlock), lds, (hipStream_t)stream, s->d_blob, s->off_grid, B, N, K, H, M, *st, mean, o, *p, q, out->n_steps, out->seg_reward, g.cpg, g.groups, g.tiles, std, *dr);
    });
}

// atc_lookahead_policy: the checks in the header's order — the pointers, then K, H, M, the mode, the policy's fields, the batch shape, and the
// overlap rule on pointer values — then k_lookahead_policy through the candidate kernels' one launch
int atc_lookahead_policy(const atc_scenario_t* s, int B, int N, int K, int H, int M, const atc_state_t* st, const float* obs0, const float* first,
                         const atc_policy_t* pol, const atc_lookahead_policy_out_t* out, const atc_params_t* p, void* stream) {
    if (!pol) return fail_arg("null pointer: pol (atc_policy_t) is required");
    if (!pol->w) return fail_arg("null pointer: pol->w (the policy's weights) is required");
    if (!out) return fail_arg("null pointer: out (atc_lookahead_policy_out_t) is required");
    if (!out->reward || !out->done) return fail_arg("null pointer: atc_lookahead_policy_out_t.reward and .done are required");
    if (!first && !obs0) return fail_arg("null pointer: obs0 is required where first is NULL (segment 0's decision reads it)");
    if (!s || !st || !p) return fail_arg("null pointer");
    if (state_has_null(st)) return fail_arg("atc_state_t has a null field");
    if (K < 1 || K > ATC_SKIP_MAX) return fail_arg("K (the segment length) must be 1 .. 255");
    if (const int rc = check_plan_h(H)) return rc;
    if (M < 1 || M > ATC_SAMPLE_MAX_M) return fail_arg("M (the number of candidates) must be 1 .. 1024");
    if (p->mode & ATC_M_DISCRETE) return fail_arg("ATC_M_DISCRETE: a Gaussian policy draws the continuous action space only");
    if (p->mode & ATC_M_ACTIONS_HELD) return fail_arg("ATC_M_ACTIONS_HELD is for atc_step only: every segment's first step carries a fresh decision");
    if (pol->n_hidden != ATC_POLICY_HIDDEN) return fail_arg("pol->n_hidden must be 64 (ATC_POLICY_HIDDEN)");
    if (pol->flags & ~ATC_POLICY_DETERMINISTIC) return fail_arg("pol->flags has unknown bits (ATC_POLICY_DETERMINISTIC or 0)");
    if (const int rc = check_batch_range(B, N)) return rc;
    if (const int rc = check_batch_size(B, N)) return rc;
    if ((unsigned long long)M * (unsigned long long)B * (unsigned long long)N >= (1ull << 32))
        return fail_arg("M*B*N must stay below 2^32 (the aircraft index of a decision's key): split the candidates");
    const uintptr_t b = (uintptr_t)B, bn = b * (uintptr_t)N, mb = (uintptr_t)M * b, mbn = (uintptr_t)M * bn, h = (uintptr_t)H;
    const ByteRange weights = {pol->w, ATC_POLICY_WORDS * 4u, "pol->w"};
    // (obs0 is not read where first is given: then it is no range of the call)
    const ByteRange arrays[18] = {{first ? nullptr : obs0, bn * (ATC_OBS_DIM * 4u), "obs0"}, {first, mbn * 12u, "first"}, {st->ac, bn * 16u, "st->ac"}, {st->alt, bn * 8u, "st->alt"},
                                  {st->last_act, bn * 16u, "st->last_act"}, {st->env, b * (ATC_ENV_WORDS * 4u), "st->env"}, {st->stats, b * (ATC_STAT_WORDS * 4u), "st->stats"},
                                  {st->phi_wide, bn * 32u, "st->phi_wide"},
                                  // the outputs, from index 8
                                  {out->reward, mb * 4u, "out->reward"}, {out->done, mb, "out->done"}, {out->n_steps, mb * 2u, "out->n_steps"},
                                  {out->seg_reward, mb * h * 4u, "out->seg_reward"}, {out->flags, mbn * 2u, "out->flags"}, {out->ac_reward, mbn * 4u, "out->ac_reward"},
                                  {out->min_sep, mb * 4u, "out->min_sep"}, {out->obs, mbn * (ATC_OBS_DIM * 4u), "out->obs"}, {out->flown, mbn * h * 12u, "out->flown"},
                                  {out->logp, mbn * h * 4u, "out->logp"}};
    if (const int rc = check_apart(weights, arrays + 8, 10, "the weights are read while the launch writes the other")) return rc;
    for (int o = 8; o < 18; ++o) {
        if (!arrays[o].ptr) continue;
        if (const int rc = check_apart(arrays[o], arrays, o, "it is written while the launch reads or writes the other")) return rc;
    }
    if (const int rc = check_dt(s, p)) return rc;   // (the first check that reads the sector: behind everything that is about pointer values)
    const LookPolicyTail pt = {obs0, pol->w, pol->seed, pol->decision0, pol->flags, out->flown, out->logp};
    return launch_candidates(REC_LOOKAHEAD_POLICY, s, B, N, M, out, cand_any(out), p, [&](auto w, auto full, const CandGrid& g, size_t lds, const atc_out_t& o, const StepDerived& q) {
        hipLaunchKernelGGL((k_lookahead_policy<decltype(w)::value, decltype(full)::value>), dim3(g.grid), dim3(kBlock), lds, (hipStream_t)stream, s->d_blob, s->off_grid, B, N, K, H, M, *st, first, o, *p, q, out->n_steps, out->seg_reward, g.cpg, g.groups, g.tiles, pt);
    });
}

int atc_plan_draw(const atc_scenario_t* s, int B, int N, int H, int M, const float* mean, const float* std, const atc_plan_draw_t* dr,
                  const int32_t* index, int E, float* actions, const atc_params_t* p, void* stream) {
    // H, then M, then E, before any pointer is looked at
    if (const int rc = check_drawn_plan(H, M, index && E < 1 ? "E (the rows of index) must be >= 1" : nullptr,
                                        {{s, "null pointer: s"}, need_mean(mean), need_std(std), need_dr(dr), {actions, "null pointer: actions"}, {p, "null pointer: p"}},
                                        p, B, N))
        return rc;
    const int R = index ? E : M;
    hipLaunchKernelGGL(k_plan_draw, dim3(flat_tiles(B, N), (unsigned)H, (unsigned)std::min(R, 65535)), dim3(kBlock), 0, (hipStream_t)stream, B, N, H, M, R, mean, std,
                       *dr, index, actions);
    HIP_TRY(hipGetLastError());
    ++record(REC_PLAN_DRAW)[0];
    return ATC_OK;
}

int atc_plan_refit(const atc_scenario_t* s, int B, int N, int H, int M, const float* mean, const float* std, const atc_plan_draw_t* dr,
                   const float* weight, float* new_mean, float* new_std, const atc_params_t* p, void* stream) {
    // H, then M, before any pointer is looked at
    if (const int rc = check_drawn_plan(H, M, nullptr,
                                        {{s, "null pointer: s"}, need_mean(mean), need_std(std), need_dr(dr), need_weight(weight), {new_mean, "null pointer: new_mean"},
                                         {new_std, "null pointer: new_std"}, {p, "null pointer: p"}},
                                        p, B, N))
        return rc;
    // new_mean == mean and new_std == std exactly are the in-place update, any other overlap is refused
    const uintptr_t rows = (uintptr_t)H * (uintptr_t)B * (uintptr_t)N * 12u, wts = (uintptr_t)M * (uintptr_t)B * 4u;
    const ByteRange ranges[5] = {{mean, rows, "mean"}, {std, rows, "std"}, {weight, wts, "weight"}, {new_mean, rows, "new_mean"}, {new_std, rows, "new_std"}};
    if (const int rc = check_disjoint(ranges, 5, {{0, 3}, {1, 4}}, "only new_mean == mean and new_std == std, as equal pointers, may share memory")) return rc;
    hipLaunchKernelGGL(k_plan_refit, dim3(flat_tiles(B, N), (unsigned)H), dim3(kBlock), 0, (hipStream_t)stream, B, N, H, M, mean, std, *dr, weight, new_mean, new_std);
    HIP_TRY(hipGetLastError());
    ++record(REC_PLAN_REFIT)[0];
    return ATC_OK;
}

int atc_plan_score(const atc_scenario_t* s, int B, int H, int M, const float* seg_reward, const uint16_t* n_steps, const atc_plan_score_t* sc,
                   float* score, float* weight, int32_t* top, int R, void* stream) {
    // H, then M, then R, before any pointer is looked at
    const char* const r_refusal = R < 0 || R > ATC_SCORE_MAX_TOP ? "R (the rows of top) must be 0 .. 64" : R > 0 && !top ? "R (the rows of top) > 0 needs top" : nullptr;
    if (const int rc = check_drawn_plan(H, M, r_refusal,
                                        {{s, "null pointer: s"}, {seg_reward, "null pointer: seg_reward is required"}, {sc, "null pointer: sc (atc_plan_score_t) is required"},
                                         {score, "null pointer: score is required (result and workspace)"}, need_weight(weight)}))
        return rc;
    if (sc->mode != ATC_SCORE_ELITE && sc->mode != ATC_SCORE_SOFTMAX) return fail_arg("sc->mode must be ATC_SCORE_ELITE or ATC_SCORE_SOFTMAX");
    if (sc->mode == ATC_SCORE_ELITE && (sc->elites < 1 || sc->elites > M)) return fail_arg("sc->elites must be 1 .. M");
    if (!(fabsf(sc->gamma) <= __FLT_MAX__)) return fail_arg("sc->gamma must be finite");
    if (sc->mode == ATC_SCORE_SOFTMAX && !(sc->temperature > 0.0f && sc->temperature <= __FLT_MAX__)) return fail_arg("sc->temperature must be > 0 and finite");
    if (B < 1) return fail_arg("need B >= 1");
    // any overlap is refused (n_steps may be absent, and top with R == 0)
    const uintptr_t mb = (uintptr_t)M * (uintptr_t)B;
    const ByteRange ranges[5] = {{seg_reward, mb * (uintptr_t)H * 4u, "seg_reward"}, {n_steps, mb * 2u, "n_steps"}, {score, mb * 4u, "score"}, {weight, mb * 4u, "weight"},
                                 {R > 0 ? top : nullptr, (uintptr_t)R * (uintptr_t)B * 4u, "top"}};
    if (const int rc = check_disjoint(ranges, 5, {}, "no two arrays of atc_plan_score may share memory")) return rc;
    const unsigned tiles = (unsigned)(((unsigned long long)B + kScoreBlock - 1) / kScoreBlock);
    hipLaunchKernelGGL(k_plan_score, dim3(tiles), dim3(kScoreBlock), 0, (hipStream_t)stream, B, H, M, seg_reward, n_steps, *sc, score, weight,
                       R > 0 ? top : nullptr, R);
    HIP_TRY(hipGetLastError());
    ++record(REC_PLAN_SCORE)[0];
    return ATC_OK;
}

int atc_branch(const atc_scenario_t* s, int B, int N, int K, int M, const atc_state_t* src, const float* actions, const atc_state_t* dst,
               const atc_lookahead_out_t* out, const atc_params_t* p, void* stream) {
    // K, then M, before any pointer is looked at
    if (K < 1 || K > ATC_SKIP_MAX) return fail_arg("K (the branch length) must be 1 .. 255");
    if (M < 1 || M > ATC_LOOKAHEAD_MAX_M) return fail_arg("M (the number of candidates) must be 1 .. 64");
    if (!out || !out->reward || !out->done) return fail_arg("null pointer: atc_lookahead_out_t.reward and .done are required");
    if (!dst || state_has_null(dst)) return fail_arg("null pointer: dst and its six arrays are required");
    // (pointer values only; a src the later checks refuse has no ranges to compare)
    if (src && B >= 1 && N >= 1 && N <= ATC_MAX_AIRCRAFT && states_overlap(dst, (unsigned long long)M * B, src, B, N))
        return fail_arg("dst (M*B envs) overlaps src (B envs)");
    if (B >= 1 && N >= 1 && N <= ATC_MAX_AIRCRAFT)
        if (const int rc = check_batch_size((unsigned long long)M * B, N, "M*B is not a batch size atc_step accepts (M*B*N*40 bytes must stay below 4 GiB): split the candidates"))
            return rc;
    if (!actions) return fail_arg("null pointer");
    if (const int rc = check_env_args(s, B, N, src, p)) return rc;
    if (const int rc = check_dt(s, p)) return rc;
    if (p->mode & ATC_M_ACTIONS_HELD) return fail_arg("ATC_M_ACTIONS_HELD is for atc_step only: every candidate's first step carries a fresh decision");
    // k_skip's rule for the form: obs and flags are stored by both (csrc/atc_branch.inc)
    return launch_candidates(REC_BRANCH, s, B, N, M, out, out->ac_reward || out->min_sep, p, [&](auto w, auto full, const CandGrid& g, size_t lds, const atc_out_t& o, const StepDerived& q) {
        hipLaunchKernelGGL((k_branch<decltype(w)::value, decltype(full)::value>), dim3(g.grid), dim3(kBlock), lds, (hipStream_t)stream, s->d_blob, s->off_grid, B, N, K, M, *src, actions, o, *p, q, out->n_steps, g.cpg, g.groups, g.tiles, *dst);
    });
}

int atc_state_select(const atc_scenario_t* s, int N, int B_dst, const atc_state_t* dst, int B_src, const atc_state_t* src, const int32_t* index,
                     const uint8_t* mask, void* stream) {
    if (N < 1 || N > ATC_MAX_AIRCRAFT || B_dst < 1 || B_src < 1) return fail_arg("need 1 <= N <= 64, B_dst >= 1 and B_src >= 1");
    if (!index || !dst || !src || state_has_null(dst) || state_has_null(src)) return fail_arg("null pointer");
    if (states_overlap(dst, B_dst, src, B_src, N)) return fail_arg("dst overlaps src");
    if (!s) return fail_arg("null pointer");
    for (const int B : {B_dst, B_src})
        if (const int rc = check_batch_size(B, N)) return rc;
    hipLaunchKernelGGL(k_select, dim3(step_grid(B_dst, N)), dim3(kBlock), 0, (hipStream_t)stream, N, B_dst, *dst, B_src, *src, index, mask);
    HIP_TRY(hipGetLastError());
    ++record(REC_SELECT)[0];
    return ATC_OK;
}

int atc_rollout_policy(const atc_scenario_t* s, int B, int N, int T, int hold, const atc_state_t* st, const float* obs0, const atc_policy_t* pol,
                       const atc_policy_out_t* out, const atc_params_t* p, void* stream) {
    if (const int rc = check_policy_call(s, B, N, T, hold, st, obs0, pol, out, p, "atc_policy_t", "atc_policy_out_t", nullptr, nullptr)) return rc;
    return with_width(N, [&](auto w) { return launch_policy<decltype(w)::value, 0>(s, B, N, T, hold, st, obs0, pol, out, p, (hipStream_t)stream); });
}

int atc_rollout_policy_traffic(const atc_scenario_t* s, int B, int N, int T, int hold, const atc_state_t* st, const float* obs0,
                               const atc_policy_traffic_t* pol, const atc_policy_traffic_out_t* out, const atc_params_t* p, void* stream) {
    if (const int rc = check_policy_call(s, B, N, T, hold, st, obs0, pol, out, p, "atc_policy_traffic_t", "atc_policy_traffic_out_t", pol ? &pol->traffic_k : nullptr,
                                         out ? out->traffic : nullptr))
        return rc;
    return with_width(N, [&](auto w) {
        return with_traffic_k(pol->traffic_k, [&](auto kt) {
            return launch_policy<decltype(w)::value, decltype(kt)::value>(s, B, N, T, hold, st, obs0, pol, out, p, (hipStream_t)stream);
        });
    });
}

// atc_gae and atc_gae_boot: the checks in the header's order, then k_gae, or k_gae_boot where boot and trunc are given
static int gae_call(Record rec, const atc_scenario_t* s, int B, int NV, int D, int hold, const float* reward, const uint8_t* done, const float* values,
                    const float* adv_next, const float* boot, const uint8_t* trunc, const atc_gae_t* g, const atc_gae_out_t* out, void* stream) {
    // D, hold, NV, B, before any pointer is looked at
    if (D < 1) return fail_arg("D (the number of decisions) must be >= 1");
    if (hold < 1 || hold > ATC_SKIP_MAX) return fail_arg("hold (the steps of a decision) must be 1 .. 255");
    if (NV < 1 || NV > ATC_GAE_MAX_NV) return fail_arg("NV (the value columns per env) must be 1 .. 64");
    if (B < 1) return fail_arg("need B >= 1");
    if (const int rc = check_required({{s, "null pointer: s"}, {reward, "null pointer: reward is required"}, {done, "null pointer: done is required"},
                                       {values, "null pointer: values is required"}, {g, "null pointer: g (atc_gae_t) is required"},
                                       {out, "null pointer: out (atc_gae_out_t) is required"}}))
        return rc;
    if (const int rc = check_required({{out->adv, "null pointer: out->adv is required"}, {out->ret, "null pointer: out->ret is required"}})) return rc;
    if (boot && !trunc) return fail_arg("null pointer: trunc is required where boot is given (both, or neither)");
    if (trunc && !boot) return fail_arg("null pointer: boot is required where trunc is given (both, or neither)");
    if (g->flags & ~(ATC_GAE_PER_DECISION | ATC_GAE_REWARD_PER_COLUMN)) return fail_arg("g->flags has unknown bits");
    if (!(fabsf(g->gamma) <= __FLT_MAX__)) return fail_arg("g->gamma must be finite");
    if (!(fabsf(g->lam) <= __FLT_MAX__)) return fail_arg("g->lam must be finite");
    // any overlap is refused (adv_next, boot and trunc and the three block outputs may be absent)
    const bool per_column = (g->flags & ATC_GAE_REWARD_PER_COLUMN) != 0u;
    const uintptr_t b = (uintptr_t)B, cols = b * (uintptr_t)NV, d = (uintptr_t)D, t = d * (uintptr_t)hold;
    const uintptr_t r_cols = per_column ? cols : b;
    const ByteRange ranges[11] = {{reward, t * r_cols * 4u, "reward"}, {done, t * b, "done"}, {values, (d + 1u) * cols * 4u, "values"},
                                  {adv_next, cols * 4u, "adv_next"}, {out->adv, d * cols * 4u, "adv"}, {out->ret, d * cols * 4u, "ret"},
                                  {out->block_reward, d * r_cols * 4u, "block_reward"}, {out->block_done, d * b, "block_done"},
                                  {out->block_steps, d * b, "block_steps"}, {boot, d * cols * 4u, "boot"}, {trunc, d * b, "trunc"}};
    if (const int rc = check_disjoint(ranges, 11, {}, rec == REC_GAE ? "no two arrays of atc_gae may share memory" : "no two arrays of atc_gae_boot may share memory"))
        return rc;
    const unsigned long long tiles = ((unsigned long long)cols + kGaeBlock - 1) / kGaeBlock;
    if (tiles > 0x7fffffffull) return fail_arg("B * NV is more than one launch covers: split the batch");
    if (boot)
        hipLaunchKernelGGL(k_gae_boot, dim3((unsigned)tiles), dim3(kGaeBlock), 0, (hipStream_t)stream, B, NV, D, hold, reward, done, values, adv_next, boot, trunc, *g, *out);
    else
        hipLaunchKernelGGL(k_gae, dim3((unsigned)tiles), dim3(kGaeBlock), 0, (hipStream_t)stream, B, NV, D, hold, reward, done, values, adv_next, *g, *out);
    HIP_TRY(hipGetLastError());
    ++record(rec)[0];
    return ATC_OK;
}

int atc_rollout_policy_ends(const atc_scenario_t* s, int B, int N, int T, int hold, const atc_state_t* st, const float* obs0,
                            const atc_policy_traffic_t* pol, const atc_policy_ends_out_t* out, const atc_params_t* p, void* stream) {
    const PolicyEnds ends = {out ? out->term_obs : nullptr, out ? out->term_flags : nullptr, out ? out->control : nullptr};
    if (const int rc = check_policy_call(s, B, N, T, hold, st, obs0, pol, out, p, "atc_policy_traffic_t", "atc_policy_ends_out_t", pol ? &pol->traffic_k : nullptr,
                                         out ? out->traffic : nullptr, &ends))
        return rc;
    return with_width(N, [&](auto w) {
        return with_traffic_k0(pol->traffic_k, [&](auto kt) {
            return launch_policy<decltype(w)::value, decltype(kt)::value, true, false>(s, B, N, T, hold, st, obs0, pol, out, p, (hipStream_t)stream);
        });
    });
}

int atc_rollout_policy_term(const atc_scenario_t* s, int B, int N, int T, int hold, const atc_state_t* st, const float* obs0,
                            const atc_policy_traffic_t* pol, const atc_policy_term_out_t* out, const atc_params_t* p, void* stream) {
    if (const int rc = check_policy_term_call(s, B, N, T, hold, st, obs0, pol, out, p)) return rc;
    return with_width(N, [&](auto w) {
        return with_traffic_k(pol->traffic_k, [&](auto kt) {
            return launch_policy<decltype(w)::value, decltype(kt)::value, true, true>(s, B, N, T, hold, st, obs0, pol, out, p, (hipStream_t)stream);
        });
    });
}

int atc_policy_eval(const atc_scenario_t* s, int B, int N, int T, int hold, const atc_state_t* st, const float* obs0, const atc_policy_traffic_t* pol,
                    const atc_policy_eval_out_t* out, const atc_params_t* p, void* stream) {
    if (const int rc = check_policy_eval_call(s, B, N, T, hold, st, obs0, pol, out, p)) return rc;
    return with_width(N, [&](auto w) {
        return with_traffic_k0(pol->traffic_k, [&](auto kt) {
            return launch_policy_eval<decltype(w)::value, decltype(kt)::value>(s, B, N, T, hold, st, obs0, pol, out, p, (hipStream_t)stream);
        });
    });
}

int atc_gae(const atc_scenario_t* s, int B, int NV, int D, int hold, const float* reward, const uint8_t* done, const float* values,
            const float* adv_next, const atc_gae_t* g, const atc_gae_out_t* out, void* stream) {
    return gae_call(REC_GAE, s, B, NV, D, hold, reward, done, values, adv_next, nullptr, nullptr, g, out, stream);
}

int atc_gae_boot(const atc_scenario_t* s, int B, int NV, int D, int hold, const float* reward, const uint8_t* done, const float* values,
                 const float* adv_next, const float* boot, const uint8_t* trunc, const atc_gae_t* g, const atc_gae_out_t* out, void* stream) {
    return gae_call(REC_GAE_BOOT, s, B, NV, D, hold, reward, done, values, adv_next, boot, trunc, g, out, stream);
}

// atc_ppo_policy_grad: the checks in the header's order, then k_ppo_grad<K> on G workgroups and k_ppo_grad_reduce, both on `stream`
int atc_ppo_policy_grad(const atc_scenario_t* s, int R_src, int R, const float* w, const float* obs_rows, const float* traffic, const float* action,
                        const float* logp_old, const float* adv, const uint8_t* mask, const int32_t* index, const atc_ppo_grad_t* g,
                        const atc_ppo_grad_out_t* out, void* stream) {
    if (const int rc = check_required({{s, "null pointer: s"}, {w, "null pointer: w (the policy's weights) is required"}, {obs_rows, "null pointer: obs_rows is required"},
                                       {action, "null pointer: action is required"}, {logp_old, "null pointer: logp_old is required"},
                                       {adv, "null pointer: adv is required"}, {g, "null pointer: g (atc_ppo_grad_t) is required"},
                                       {out, "null pointer: out (atc_ppo_grad_out_t) is required"}}))
        return rc;
    if (const int rc = check_required({{out->grad, "null pointer: out->grad is required"}, {out->stats, "null pointer: out->stats is required"},
                                       {out->scratch, "null pointer: out->scratch is required"}}))
        return rc;
    const int K = g->traffic_k;
    if (K != 0 && K != 1 && K != 2 && K != 4) return fail_arg("g->traffic_k must be 0, 1, 2 or 4 (the ten-word policy, or a compiled list length)");
    if (R_src < 1) return fail_arg("R_src (the number of source rows) must be >= 1");
    if (R < 1) return fail_arg("R (the number of rows to evaluate) must be >= 1");
    if (!index && R != R_src) return fail_arg("R must equal R_src where index is NULL (the identity)");
    if (!(g->clip > 0.0f && g->clip <= __FLT_MAX__)) return fail_arg("g->clip must be finite and > 0");
    if (g->workgroups < 0 || g->workgroups > ATC_PPO_GRAD_MAX_WG) return fail_arg("g->workgroups must be 0 (the library's choice) .. 1024 (ATC_PPO_GRAD_MAX_WG)");
    if (K > 0 && !traffic) return fail_arg("null pointer: traffic is required where g->traffic_k > 0");
    if (K == 0 && traffic) return fail_arg("traffic must be NULL where g->traffic_k is 0 (the ten-word policy reads no records)");
    const long long tiles = ((long long)R + (kPpoBlock - 1)) / kPpoBlock;
    const int G = g->workgroups ? g->workgroups : (int)(tiles < ATC_PPO_GRAD_DEFAULT_WG ? tiles : ATC_PPO_GRAD_DEFAULT_WG);
    const int words = ATC_POLICY_TRAFFIC_WORDS(K);
    // no output may share memory with any array of the call (the inputs may share among themselves)
    const uintptr_t rs = (uintptr_t)R_src, r = (uintptr_t)R;
    const ByteRange outputs[4] = {{out->grad, (uintptr_t)words * 4u, "grad"}, {out->stats, ATC_PPO_GRAD_STATS * 4u, "stats"}, {out->logp_new, r * 4u, "logp_new"},
                                  {out->scratch, (uintptr_t)G * (uintptr_t)(words + ATC_PPO_GRAD_STATS) * 4u, "scratch"}};
    const ByteRange inputs[8] = {{w, (uintptr_t)words * 4u, "w"}, {obs_rows, rs * (ATC_OBS_DIM * 4u), "obs_rows"},
                                 {traffic, rs * (uintptr_t)K * (ATC_TRAFFIC_DIM * 4u), "traffic"}, {action, rs * 12u, "action"}, {logp_old, rs * 4u, "logp_old"},
                                 {adv, rs * 4u, "adv"}, {mask, rs, "mask"}, {index, r * 4u, "index"}};
    for (int a = 0; a < 4; ++a) {
        if (!outputs[a].ptr) continue;
        for (int b = 0; b < 8 + a; ++b) {
            const ByteRange pair[2] = {b < 8 ? inputs[b] : outputs[b - 8], outputs[a]};
            if (const int rc = check_disjoint(pair, 2, {}, "no output of atc_ppo_policy_grad may share memory with another array")) return rc;
        }
    }
    const atc_ppo_grad_t gp = *g;
    with_traffic_k0(K, [&](auto kt) {
        hipLaunchKernelGGL(k_ppo_grad<decltype(kt)::value>, dim3((unsigned)G), dim3(kPpoBlock), 0, (hipStream_t)stream, R_src, R, w, obs_rows, traffic, action, logp_old,
                           adv, mask, index, gp, out->logp_new, out->scratch);
        return ATC_OK;
    });
    HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(k_ppo_grad_reduce, dim3((unsigned)((words + ATC_PPO_GRAD_STATS + kPpoReduceBlock - 1) / kPpoReduceBlock)), dim3(kPpoReduceBlock), 0,
                       (hipStream_t)stream, words, G, out->scratch, out->grad, out->stats);
    HIP_TRY(hipGetLastError());
    ++record(REC_PPO_GRAD)[K ? 1 + __builtin_ctz(K) : 0];
    return ATC_OK;
}

// atc_value_forward: the checks in the header's order, then k_value_forward<K> on `stream`, one lane per row
int atc_value_forward(const atc_scenario_t* s, int R, int traffic_k, const float* w, const float* x, float* values, void* stream) {
    if (const int rc = check_required({{s, "null pointer: s"}, {w, "null pointer: w (the critic's weights) is required"}, {x, "null pointer: x (the input rows) is required"},
                                       {values, "null pointer: values is required"}}))
        return rc;
    if (R < 1) return fail_arg("R (the number of rows) must be >= 1");
    const int K = traffic_k;
    if (K != 0 && K != 1 && K != 2 && K != 4) return fail_arg("traffic_k must be 0, 1, 2 or 4 (the ten-word row, or a compiled list length)");
    const uintptr_t r = (uintptr_t)R;
    const ByteRange out = {values, r * 4u, "values"};
    const ByteRange inputs[2] = {{x, r * (uintptr_t)ATC_POLICY_TRAFFIC_IN(K) * 4u, "x"}, {w, (uintptr_t)ATC_VALUE_WORDS(K) * 4u, "w"}};
    for (int b = 0; b < 2; ++b) {
        const ByteRange pair[2] = {inputs[b], out};
        if (const int rc = check_disjoint(pair, 2, {}, "values of atc_value_forward may not share memory with its inputs")) return rc;
    }
    const unsigned blocks = (unsigned)(((long long)R + (kValueBlock - 1)) / kValueBlock);
    with_traffic_k0(K, [&](auto kt) {
        hipLaunchKernelGGL(k_value_forward<decltype(kt)::value>, dim3(blocks), dim3(kValueBlock), 0, (hipStream_t)stream, R, w, x, values);
        return ATC_OK;
    });
    HIP_TRY(hipGetLastError());
    ++record(REC_VALUE_FORWARD)[K ? 1 + __builtin_ctz(K) : 0];
    return ATC_OK;
}

// atc_policy_forward: the checks in the header's order, then k_policy_forward<K> on `stream`, one lane per row
int atc_policy_forward(const atc_scenario_t* s, int R, const float* w, const float* obs_rows, const float* traffic, const atc_policy_fwd_t* f,
                       const atc_policy_fwd_out_t* out, void* stream) {
    if (const int rc = check_required({{s, "null pointer: s"}, {w, "null pointer: w (the policy's weights) is required"}, {obs_rows, "null pointer: obs_rows is required"},
                                       {f, "null pointer: f (atc_policy_fwd_t) is required"}, {out, "null pointer: out (atc_policy_fwd_out_t) is required"}}))
        return rc;
    const int K = f->traffic_k;
    if (K != 0 && K != 1 && K != 2 && K != 4) return fail_arg("f->traffic_k must be 0, 1, 2 or 4 (the ten-word policy, or a compiled list length)");
    if (R < 1) return fail_arg("R (the number of rows) must be >= 1");
    const int S = f->samples;
    if (S < 1 || S > ATC_POLICY_FWD_MAX_SAMPLES) return fail_arg("f->samples must be 1 .. 64 (ATC_POLICY_FWD_MAX_SAMPLES)");
    if (f->rows_per_decision < 0 || f->rows_per_decision > R) return fail_arg("f->rows_per_decision must be 1 .. R, or 0 for R");
    if ((f->flags & ATC_POLICY_DETERMINISTIC) && S > 1) return fail_arg("ATC_POLICY_DETERMINISTIC draws nothing: f->samples must be 1");
    if (f->flags & ~ATC_POLICY_DETERMINISTIC) return fail_arg("f->flags has unknown bits");
    if (K > 0 && !traffic) return fail_arg("null pointer: traffic is required where f->traffic_k > 0");
    if (K == 0 && traffic) return fail_arg("traffic must be NULL where f->traffic_k is 0 (the ten-word policy reads no records)");
    if (!out->mean && !out->action && !out->flown && !out->logp) return fail_arg("null pointer: out names no output (mean, action, flown, logp)");
    // no output may share memory with any array of the call (the inputs may share among themselves)
    const uintptr_t r = (uintptr_t)R, sr = (uintptr_t)S * r;
    const ByteRange outputs[4] = {{out->mean, r * 12u, "mean"}, {out->action, sr * 12u, "action"}, {out->flown, sr * 12u, "flown"}, {out->logp, sr * 4u, "logp"}};
    const ByteRange inputs[3] = {{w, (uintptr_t)ATC_POLICY_TRAFFIC_WORDS(K) * 4u, "w"}, {obs_rows, r * (ATC_OBS_DIM * 4u), "obs_rows"},
                                 {traffic, r * (uintptr_t)K * (ATC_TRAFFIC_DIM * 4u), "traffic"}};
    for (int a = 0; a < 4; ++a) {
        if (!outputs[a].ptr) continue;
        for (int b = 0; b < 3 + a; ++b) {
            const ByteRange pair[2] = {b < 3 ? inputs[b] : outputs[b - 3], outputs[a]};
            if (const int rc = check_disjoint(pair, 2, {}, "no output of atc_policy_forward may share memory with another array")) return rc;
        }
    }
    const uint32_t P = f->rows_per_decision ? (uint32_t)f->rows_per_decision : (uint32_t)R;
    const PolicyFwdDraw dr = {f->seed, f->decision0, (uint32_t)(((unsigned long long)R + P - 1u) / P), P, S, f->flags};
    const unsigned blocks = (unsigned)(((long long)R + (kPolFwdBlock - 1)) / kPolFwdBlock);
    with_traffic_k0(K, [&](auto kt) {
        hipLaunchKernelGGL(k_policy_forward<decltype(kt)::value>, dim3(blocks), dim3(kPolFwdBlock), 0, (hipStream_t)stream, R, w, obs_rows, traffic, dr, out->mean,
                           out->action, out->flown, out->logp);
        return ATC_OK;
    });
    HIP_TRY(hipGetLastError());
    ++record(REC_POLICY_FORWARD)[K ? 1 + __builtin_ctz(K) : 0];
    return ATC_OK;
}

// atc_ppo_value_grad: the checks in the header's order, then k_ppo_value_grad<K> on G workgroups and k_ppo_value_grad_reduce, both on `stream`
int atc_ppo_value_grad(const atc_scenario_t* s, int R_src, int R, int traffic_k, const float* w, const float* obs_rows, const float* traffic, const float* v_old,
                       const float* ret, const uint8_t* mask, const int32_t* index, const atc_ppo_value_grad_t* g, const atc_ppo_value_grad_out_t* out,
                       void* stream) {
    if (const int rc = check_required({{s, "null pointer: s"}, {w, "null pointer: w (the critic's weights) is required"}, {obs_rows, "null pointer: obs_rows is required"},
                                       {v_old, "null pointer: v_old is required"}, {ret, "null pointer: ret is required"},
                                       {g, "null pointer: g (atc_ppo_value_grad_t) is required"}, {out, "null pointer: out (atc_ppo_value_grad_out_t) is required"}}))
        return rc;
    if (const int rc = check_required({{out->grad, "null pointer: out->grad is required"}, {out->stats, "null pointer: out->stats is required"},
                                       {out->scratch, "null pointer: out->scratch is required"}}))
        return rc;
    const int K = traffic_k;
    if (K != 0 && K != 1 && K != 2 && K != 4) return fail_arg("traffic_k must be 0, 1, 2 or 4 (the ten-word row, or a compiled list length)");
    if (R_src < 1) return fail_arg("R_src (the number of source rows) must be >= 1");
    if (R < 1) return fail_arg("R (the number of rows to evaluate) must be >= 1");
    if (!index && R != R_src) return fail_arg("R must equal R_src where index is NULL (the identity)");
    if (!(g->clip > 0.0f)) return fail_arg("g->clip must be > 0 (+inf: no clipping) and not a NaN");
    if (g->workgroups < 0 || g->workgroups > ATC_PPO_GRAD_MAX_WG) return fail_arg("g->workgroups must be 0 (the library's choice) .. 1024 (ATC_PPO_GRAD_MAX_WG)");
    if (K > 0 && !traffic) return fail_arg("null pointer: traffic is required where traffic_k > 0");
    if (K == 0 && traffic) return fail_arg("traffic must be NULL where traffic_k is 0 (the ten-word row has no records)");
    const long long tiles = ((long long)R + (kPpoBlock - 1)) / kPpoBlock;
    const int G = g->workgroups ? g->workgroups : (int)(tiles < ATC_PPO_GRAD_DEFAULT_WG ? tiles : ATC_PPO_GRAD_DEFAULT_WG);
    const int words = ATC_VALUE_WORDS(K);
    // no output may share memory with any array of the call (the inputs may share among themselves)
    const uintptr_t rs = (uintptr_t)R_src, r = (uintptr_t)R;
    const ByteRange outputs[4] = {{out->grad, (uintptr_t)words * 4u, "grad"}, {out->stats, ATC_PPO_VALUE_STATS * 4u, "stats"}, {out->value, r * 4u, "value"},
                                  {out->scratch, (uintptr_t)G * (uintptr_t)(words + ATC_PPO_VALUE_STATS) * 4u, "scratch"}};
    const ByteRange inputs[7] = {{w, (uintptr_t)words * 4u, "w"}, {obs_rows, rs * (ATC_OBS_DIM * 4u), "obs_rows"},
                                 {traffic, rs * (uintptr_t)K * (ATC_TRAFFIC_DIM * 4u), "traffic"}, {v_old, rs * 4u, "v_old"}, {ret, rs * 4u, "ret"},
                                 {mask, rs, "mask"}, {index, r * 4u, "index"}};
    for (int a = 0; a < 4; ++a) {
        if (!outputs[a].ptr) continue;
        for (int b = 0; b < 7 + a; ++b) {
            const ByteRange pair[2] = {b < 7 ? inputs[b] : outputs[b - 7], outputs[a]};
            if (const int rc = check_disjoint(pair, 2, {}, "no output of atc_ppo_value_grad may share memory with another array")) return rc;
        }
    }
    const float clip = g->clip;
    with_traffic_k0(K, [&](auto kt) {
        hipLaunchKernelGGL(k_ppo_value_grad<decltype(kt)::value>, dim3((unsigned)G), dim3(kPpoBlock), 0, (hipStream_t)stream, R_src, R, w, obs_rows, traffic, v_old, ret,
                           mask, index, clip, out->value, out->scratch);
        return ATC_OK;
    });
    HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(k_ppo_value_grad_reduce, dim3((unsigned)((words + ATC_PPO_VALUE_STATS + kPpoReduceBlock - 1) / kPpoReduceBlock)), dim3(kPpoReduceBlock), 0,
                       (hipStream_t)stream, words, G, out->scratch, out->grad, out->stats);
    HIP_TRY(hipGetLastError());
    ++record(REC_PPO_VALUE_GRAD)[K ? 1 + __builtin_ctz(K) : 0];
    return ATC_OK;
}

// atc_adv_normalise: the checks in the header's order, then k_adv_moments on G workgroups and k_adv_apply, both on `stream`
int atc_adv_normalise(const atc_scenario_t* s, int R, const float* adv, const uint8_t* mask, const atc_adv_norm_t* g, const atc_adv_norm_out_t* out,
                      void* stream) {
    if (const int rc = check_required({{s, "null pointer: s"}, {adv, "null pointer: adv is required"}, {g, "null pointer: g (atc_adv_norm_t) is required"},
                                       {out, "null pointer: out (atc_adv_norm_out_t) is required"}}))
        return rc;
    if (const int rc = check_required({{out->stats, "null pointer: out->stats is required"}, {out->scratch, "null pointer: out->scratch is required"}})) return rc;
    if (R < 1) return fail_arg("R (the number of rows) must be >= 1");
    if (!(g->eps >= 0.0f && g->eps <= __FLT_MAX__)) return fail_arg("g->eps must be finite and >= 0");
    if (g->workgroups < 0 || g->workgroups > ATC_ADV_MAX_WG) return fail_arg("g->workgroups must be 0 (the library's choice) .. 1024 (ATC_ADV_MAX_WG)");
    const long long tiles = ((long long)R + (kAdvBlock - 1)) / kAdvBlock;
    const int G = g->workgroups ? g->workgroups : (int)(tiles < ATC_ADV_DEFAULT_WG ? tiles : ATC_ADV_DEFAULT_WG);
    // no output may share memory with any array of the call; out_adv may BE adv (the one in-place pair)
    const uintptr_t r = (uintptr_t)R;
    const ByteRange arrays[5] = {{adv, r * 4u, "adv"}, {mask, r, "mask"}, {out->out_adv, r * 4u, "out_adv"}, {out->stats, ATC_ADV_STATS * 4u, "stats"},
                                 {out->scratch, (uintptr_t)G * 24u, "scratch"}};
    for (int a = 2; a < 5; ++a)
        for (int b = 0; b < a; ++b) {
            if (a == 2 && b == 0 && adv == out->out_adv) continue;
            const ByteRange pair[2] = {arrays[b], arrays[a]};
            if (const int rc = check_disjoint(pair, 2, {}, "no output of atc_adv_normalise may share memory with another array; out_adv may be adv itself")) return rc;
        }
    hipLaunchKernelGGL(k_adv_moments, dim3((unsigned)G), dim3(kAdvBlock), 0, (hipStream_t)stream, R, adv, mask, out->scratch);
    HIP_TRY(hipGetLastError());
    const unsigned grid = (unsigned)(tiles < kAdvApplyMaxGrid ? tiles : kAdvApplyMaxGrid);
    hipLaunchKernelGGL(k_adv_apply, dim3(out->out_adv ? grid : 1u), dim3(kAdvBlock), 0, (hipStream_t)stream, R, G, g->eps, adv, mask,
                       (const double*)out->scratch, out->out_adv, out->stats);
    HIP_TRY(hipGetLastError());
    ++record(REC_ADV_NORMALISE)[0];
    return ATC_OK;
}

// atc_adam_step: the checks in the header's order, then k_adam_step, one workgroup on `stream`
int atc_adam_step(const atc_scenario_t* s, int n_tensors, const atc_adam_tensor_t* t, const atc_adam_t* g, float* stats, void* stream) {
    if (const int rc = check_required({{s, "null pointer: s"}, {t, "null pointer: t (atc_adam_tensor_t) is required"}, {g, "null pointer: g (atc_adam_t) is required"},
                                       {stats, "null pointer: stats is required"}}))
        return rc;
    if (n_tensors != 1 && n_tensors != 2) return fail_arg("n_tensors must be 1 or 2");
    auto finite = [](double x) { return x - x == 0.0; };
    for (int k = 0; k < n_tensors; ++k) {
        if (!t[k].w || !t[k].grad || !t[k].m || !t[k].v) return fail_argf("null pointer: w, grad, m and v of tensor %d are required", k);
        if (t[k].words < 1 || t[k].words > ATC_ADAM_MAX_WORDS) return fail_argf("words of tensor %d must be 1 .. 65536 (ATC_ADAM_MAX_WORDS)", k);
        if (t[k].add_count < 0 || (t[k].add_count > 0 && (t[k].add_first < 0 || (long long)t[k].add_first + t[k].add_count > t[k].words)))
            return fail_argf("the add window of tensor %d must lie inside the tensor (add_first >= 0, add_first + add_count <= words), or add_count be 0", k);
        if (!finite(t[k].grad_scale) || !finite(t[k].add_value)) return fail_argf("grad_scale and add_value of tensor %d must be finite", k);
    }
    if (g->step < 1) return fail_arg("g->step must be >= 1 (the number of this update, counted from 1)");
    if (!finite(g->lr) || g->lr < 0.0) return fail_arg("g->lr must be finite and >= 0");
    if (!finite(g->eps) || g->eps < 0.0) return fail_arg("g->eps must be finite and >= 0");
    if (!(g->beta1 >= 0.0 && g->beta1 < 1.0) || !(g->beta2 >= 0.0 && g->beta2 < 1.0)) return fail_arg("g->beta1 and g->beta2 must lie in [0, 1)");
    if (g->max_norm != g->max_norm) return fail_arg("g->max_norm must not be a NaN (<= 0 or +inf: no clip)");
    // every array of the call is read and written in place: none may share memory with another
    ByteRange arrays[9];
    static const char* const names[2][4] = {{"w of tensor 0", "grad of tensor 0", "m of tensor 0", "v of tensor 0"},
                                            {"w of tensor 1", "grad of tensor 1", "m of tensor 1", "v of tensor 1"}};
    int n = 0;
    for (int k = 0; k < n_tensors; ++k) {
        const void* ptr[4] = {t[k].w, t[k].grad, t[k].m, t[k].v};
        for (int a = 0; a < 4; ++a) arrays[n++] = ByteRange{ptr[a], (uintptr_t)t[k].words * 4u, names[k][a]};
    }
    arrays[n++] = ByteRange{stats, ATC_ADAM_STATS * 4u, "stats"};
    if (const int rc = check_disjoint(arrays, n, {}, "atc_adam_step updates in place: no two of its arrays may share memory")) return rc;
    AdamArgs a = {};
    for (int k = 0; k < n_tensors; ++k)
        a.t[k] = AdamTensorArg{t[k].w, t[k].grad, t[k].m, t[k].v, t[k].words, t[k].grad_scale, t[k].add_first, t[k].add_count, t[k].add_value};
    a.lr = g->lr;
    a.beta1 = g->beta1;
    a.beta2 = g->beta2;
    a.eps = g->eps;
    a.max_norm = g->max_norm;
    a.c1 = 1.0 - pow(g->beta1, (double)g->step);
    a.c2 = 1.0 - pow(g->beta2, (double)g->step);
    a.step = g->step;
    hipLaunchKernelGGL(k_adam_step, dim3(1), dim3(kAdamBlock), 0, (hipStream_t)stream, a, stats);
    HIP_TRY(hipGetLastError());
    ++record(REC_ADAM_STEP)[n_tensors - 1];
    return ATC_OK;
}

}  // extern "C"
