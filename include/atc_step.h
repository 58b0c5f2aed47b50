/*
 * atc_step.h — C-ABI of libatcstep.so, the MI355X (gfx950) implementation of the batched
 * AtcGym.step() hot path of fvalka/atc-reinforcement-learning.
 *
 * The reference has no FFI (pure Python).  Each entry point below replaces a Python call site of the
 * reference (cited as path:line relative to the reference tree) and is what a ctypes binding on the
 * reference side would load (see INTEGRATION.md for the stub).
 *
 * Conventions
 *   - extern "C", plain pointers and sizes.  No exceptions, no Python/torch objects cross the boundary.
 *   - every int-returning function: 0 = ok, ATC_ERR_* (<0) otherwise; atc_last_error() gives a
 *     thread-local message.
 *   - every buffer is a BORROWED device pointer (e.g. torch tensor .data_ptr()); the library owns only
 *     the opaque scenario handle.
 *   - all launches are asynchronous on the caller's HIP stream (`stream` = hipStream_t, e.g.
 *     torch.cuda.current_stream().cuda_stream); the caller synchronises.
 *   - aircraft arrays are SoA, index = env * N + k   (k = aircraft slot in the env, N <= 64).
 *   - re-entrant: no global mutable state besides the thread-local error string.
 */
#ifndef ATC_STEP_H
#define ATC_STEP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* The ABI number guards what a caller built against another version of this header would get WRONG IN MEMORY: it moves when a record
 * layout, a blob word, a struct or the signature of an existing entry point changes (18, 19, 20, 22 each changed a record).  It does not
 * move for a new entry point, nor for a change of documented behaviour that leaves every layout and signature as it is — such a change
 * is stated where the behaviour is described (e.g. "NON-FINITE ACTIONS" below). */
#define ATC_ABI_VERSION 22

/* ---------------------------------------------------------------------------------------------
 * Scenario blob: one flat array of 32-bit floats (device copy) compiled on the host from the sector
 * description (reference: envs/atc/scenarios.py:14-207, envs/atc/model.py:148-186,260-306,
 * envs/atc/atc_gym.py:45-58,88-110).  Integer fields are stored as exactly representable floats.
 * The float64 master (used by the f64 oracle) has the identical word layout.
 * ------------------------------------------------------------------------------------------- */
#define ATC_BLOB_VERSION 1014.0f
enum {
    ATC_H_VERSION = 0,   /* ATC_BLOB_VERSION */
    ATC_H_NWORDS = 1,    /* total words */
    ATC_H_N_MVA = 2,     /* number of MVA polygons (list order = lookup priority, model.py:283) */
    ATC_H_N_NOISE = 3,   /* number of noise-abatement polygons (extension; 0 for reference scenarios) */
    ATC_H_N_ENTRY = 4,   /* number of entry points (scenarios.py:192-207) */
    ATC_H_OFF_POLY = 5,  /* word offset of polygon table: MVA polygons first, then noise polygons */
    ATC_H_OFF_VERT = 6,  /* word offset of vertex pool (x,y interleaved; rings closed: first == last) */
    ATC_H_OFF_ENTRY = 7, /* word offset of entry-point table */
    ATC_H_OFF_GRID = 8,  /* word offset of the MVA lookup grid (0 = absent) */
    ATC_H_N_VERTW = 9,   /* words in the vertex pool */
    ATC_H_OFF_SLOT = 10, /* word offset of the slot-lattice spawn table: 64 x (x, y, phi, h) for aircraft slot k =
                            entry k mod n_entry at level (k div n_entry) mod n_levels (the non-random reset) */
    ATC_H_OFF_SPAWN = 11,/* word offset (64-byte aligned) of the device's SPAWN RECORDS, ATC_SPAWN_WORDS words each: 64 records
                            for the slot lattice (record k = aircraft slot k), then one per entry point (random resets; the
                            altitude of those comes from the drawn level).  A record is what AtcGym.reset computes for an
                            aircraft placed there (atc_gym.py:346-351,365), evaluated once on the host:
                              words 0..3   x_fix, y_fix (position grid counts), h (float), phi_fix (heading counts) — 32-bit
                                           PATTERNS in the fp32 device blob (integers are not stored as float values here)
                              words 4..13  the RAW reset observation _get_state(mva = 0), atc_gym.py:262-277,351
                              words 14..15 0
                            The float64 master holds the same quantities as values (nothing reads them there). */
    /* constants block */
    ATC_C_RWY_X = 16, ATC_C_RWY_Y = 17, ATC_C_RWY_H = 18,
    ATC_C_PHI_TO_RWY = 19,                /* (phi_from_runway + 180) % 360, model.py:163,245 */
    ATC_C_FAF_X = 20, ATC_C_FAF_Y = 21,   /* model.py:171-172 */
    ATC_C_NRM_X = 22, ATC_C_NRM_Y = 23,   /* _faf_iaf_normal, model.py:164 */
    ATC_C_FAF_ANGLE = 24,                 /* 45, model.py:167 */
    ATC_C_GS_TAN = 25,                    /* tan(3*pi/180), model.py:204 */
    ATC_C_FAF_MVA = 26,                   /* atc_gym.py:49 */
    ATC_C_WORLD_DIAG = 27,                /* atc_gym.py:58 */
    ATC_C_NM_TO_FT = 28,                  /* 6076, model.py:10 */
    ATC_C_V_MIN = 29, ATC_C_V_MAX = 30, ATC_C_H_MIN = 31, ATC_C_H_MAX = 32,          /* model.py:13 */
    ATC_C_A_MIN = 33, ATC_C_A_MAX = 34, ATC_C_HDOT_MIN = 35, ATC_C_HDOT_MAX = 36,     /* model.py:45-48 */
    ATC_C_PHIDOT_MIN = 37, ATC_C_PHIDOT_MAX = 38, ATC_C_V_INIT = 39,                  /* model.py:49-50; atc_gym.py:348 */
    ATC_C_TRI_H = 40,   /* corridor_horizontal ring [faf, corner1, corner2, faf], 8 words, model.py:177 */
    ATC_C_TRI_1 = 48,   /* corridor1 ring [faf, corner1, iaf, faf], model.py:180 */
    ATC_C_TRI_2 = 56,   /* corridor2 ring [faf, corner2, iaf, faf], model.py:181 */
    ATC_C_NORM_MIN = 64,  /* 10 words, atc_gym.py:88-98 */
    ATC_C_NORM_MAX = 74,  /* 10 words, atc_gym.py:99-110 */
    ATC_C_ACT_DISCR = 84, /* 3 words (5, 50, 0.5), atc_gym.py:84 */
    ATC_C_BBOX = 87,      /* x0,y0,x1,y1, model.py:294-301 */
    ATC_C_DIR_RWY_X = 91, ATC_C_DIR_RWY_Y = 92, /* rot_matrix(phi_to_runway) . [0,1], model.py:219 */
    ATC_C_ALIGNED_OK = 93, /* 1 if the reference's angle window (model.py:216-229) accepts phi == phi_to_runway exactly,
                              evaluated on the host with the reference's own expression (np.dot / arccos) */
    /* fixed-point position grid of the fp32 path (see "Aircraft positions" below): nm = X0 + fix * 2^-k */
    ATC_C_POS_X0 = 94, ATC_C_POS_Y0 = 95, /* grid origin [nm], integer-valued */
    ATC_C_POS_SCALE = 100,                /* 2^k  (counts per nm) */
    ATC_C_POS_INV = 101,                  /* 2^-k (nm per count) */
    ATC_C_TRI_BBOX = 96,  /* x0,y0,x1,y1 of the corridor_horizontal triangle (exact early-out for model.py:198) */
    ATC_C_NORM_A = 104,   /* 10 words: 1 / (0.5 max)              — normalisation (atc_gym.py:187-189) as one fma:  */
    ATC_C_NORM_B = 114,   /* 10 words: -(min + 0.5 max) / (0.5 max)                  obs = raw * A + B (float32) */
    ATC_C_FAF_FIX = 124,  /* 4 words: the FAF on the position grid, x then y, each as (hi, lo) with fix = hi * 65536 + lo,
                             lo in [0, 65536) — two exactly representable floats per 32-bit integer */
    ATC_C_END = 128
};
/* polygon table record (8 words) */
enum { ATC_P_MINX = 0, ATC_P_MINY = 1, ATC_P_MAXX = 2, ATC_P_MAXY = 3,
       ATC_P_HEIGHT = 4,  /* MVA height [ft] (model.py:265) or noise-area ceiling [ft] */
       ATC_P_VOFF = 5,    /* word offset of first vertex */
       ATC_P_NVERT = 6,   /* number of vertices in the closed ring (= len(area_as_list)) */
       ATC_P_PENALTY = 7, /* noise-area per-step penalty (0 for MVA polygons) */
       ATC_P_WORDS = 8 };
/* entry-point record (12 words): x, y, phi, n_levels, levels[8] (flight levels, x100 ft; model.py:309-315) */
#define ATC_SPAWN_WORDS 16
enum { ATC_E_X = 0, ATC_E_Y = 1, ATC_E_PHI = 2, ATC_E_NLEV = 3, ATC_E_LEV0 = 4, ATC_E_WORDS = 12, ATC_E_MAXLEV = 8 };
/* lookup grid (optional acceleration structure for Airspace.find_mva, model.py:282-289; results identical to the
 * ordered polygon scan by construction — see atc_hip/scenario.py:build_grid).  16-byte aligned in the blob.
 *   header 8 words : x0, y0, 1/cell, nx, ny, offset of the edge pool (from grid start), number of edge records, 0
 *   cells  ny*nx*2 : (c, v) with |c| = code + 64 * noise mask (bit q: the bounds of noise-abatement area q meet the cell)
 *                    + 2^22 if the bounds of the corridor's horizontal triangle (ATC_C_TRI_BBOX) meet the cell
 *                    + 2^23 (ATC_G_CELL_LINE) if the cell is a SPLIT cell, see below
 *                    c > 0  : dirty cell, code = n_records (< 64), v = first record: walk that many edge records
 *                    c <= 0 : clean cell, code = polygon + 1 and v = MVA height — every point has this answer;
 *                             code = 0: outside the airspace
 *                    The OUTERMOST ring of cells is (0, 0) — clean, outside, no noise candidate: a point beyond the grid is
 *                    answered by the border cell its clamped index names (atc_scenario_create refuses other grids).
 *   pool           : 8-word records, two 16-byte halves G | M (flags and folding rules: atc_hip/scenario.py:build_grid):
 *                    edge       G = p1x, p1y, p2x, p2y          M = min(p1y,p2y), max(p1y,p2y), polygon height, code
 *                    terminator G = polygon bounds x0,y0,x1,y1  M = 0, 0, polygon height, code
 *                    code = 16 * polygon index + flags                                                                */
enum { ATC_G_X0 = 0, ATC_G_Y0 = 1, ATC_G_INV = 2, ATC_G_NX = 3, ATC_G_NY = 4, ATC_G_OFF_POOL = 5, ATC_G_NREC = 6,
       ATC_G_HDR = 8, ATC_GE_WORDS = 8 };
#define ATC_G_CELL_LINE (1u << 23) /* |c| flag of a SPLIT cell: its first record (not counted in `code`) is a LINE record
                                      G = p1x, p1y, dx/dy, margin   M = left polygon + 1, left height, right polygon + 1, right height:
                                      xl = p1x + (y - p1y) dx/dy;  x < xl - margin -> the left answer, x > xl + margin -> the right
                                      one (polygon + 1 = 0: outside the airspace), else walk the `code` ordinary records behind it */
#define ATC_GE_TERM 1    /* terminator: (crossing parity xor BASE) and the bounds test (model.py:286-287) decide now */
#define ATC_GE_CERTAIN 2 /* the cell lies entirely left of this edge: crossing iff the two y tests pass */
#define ATC_GE_LAST 4    /* last edge of a polygon whose bounds contain the whole cell: parity xor BASE decides now */
#define ATC_GE_BASE 8    /* an odd number of the polygon's edges is crossed by EVERY point of the cell (not listed) */

/* ---------------------------------------------------------------------------------------------
 * LDS-resident lookup table (ABI 21, optional; atc_scenario_attach_lds_table).  A second, compact form of Airspace.find_mva
 * (model.py:282-289) for the multi-step launches of ONE-aircraft envs that fit one workgroup per CU (65 536 x 1): each workgroup
 * stages the table in LDS once per launch and a step then answers from LDS instead of gathering a lookup-grid cell from global
 * memory (one wavefront per SIMD: that gather and the records behind it are 1.2 of the step's 2.9 us).  Same answers as the
 * ordered polygon scan, by the construction of the lookup grid (atc_hip/scenario.py:build_lds_table):
 *   bytes [0, 96)  : 24 header words, ATC_LDS_H_* (x0, y0, 1 / cell as fp32 patterns; offsets in bytes from the table's start)
 *   -- staged in LDS (bytes [0, ATC_LDS_H_LDS_BYTES)) --
 *   level 1        : uint16 codes [ny][nx], cells of 1 / inv nm (0.5) over the padded sector; the outermost ring is 0
 *   level 2        : uint16 codes [n_sub][8][8], the sub-cells of every level-1 cell of kind SUB
 *   LINE records   : float [n_line][8] = p1x, p1y, dx/dy, margin | left polygon + 1, height, right polygon + 1, height (ATC_G_CELL_LINE)
 *   heights        : float [64], index polygon + 1 ([0] = 0)
 *   walk words     : uint32 [n_resid] = first record | n_records << 24 of a RESID sub-cell's edge records in the pool
 *   -- read from global memory --
 *   pool           : float [n_rec][8], edge / terminator records in the lookup grid's format ("pool" above)
 *   code           : bit 15 = the cell meets the bounds of the corridor's horizontal triangle (level 1 only); bits 14..13 = kind
 *                    (ATC_LDS_CLEAN: payload = polygon + 1, 0 = outside; ATC_LDS_LINE: payload = LINE record; ATC_LDS_SUB, level 1
 *                    only: payload = sub-cell block; ATC_LDS_RESID, level 2 only: a vertex or a second border inside the sub-cell,
 *                    payload = walk word); bits 12..0 = payload
 * A lane in a RESID sub-cell walks its records (ONE trip to global memory for the lanes concerned); a point inside a LINE record's
 * margin band sends its whole wavefront to the lookup grid for that step, so the table is only attached to a scenario that HAS a
 * grid — and has no noise-abatement areas (the codes carry no candidate masks).  Results are identical with and without the table.
 * ------------------------------------------------------------------------------------------- */
#define ATC_LDS_MAGIC 0x3154444Cu /* "LDT1" */
enum { ATC_LDS_H_MAGIC = 0, ATC_LDS_H_BYTES = 1, ATC_LDS_H_X0 = 2, ATC_LDS_H_Y0 = 3, ATC_LDS_H_INV = 4, ATC_LDS_H_NX = 5,
       ATC_LDS_H_NY = 6, ATC_LDS_H_OFF_L1 = 7, ATC_LDS_H_OFF_SUB = 8, ATC_LDS_H_N_SUB = 9, ATC_LDS_H_OFF_LINE = 10,
       ATC_LDS_H_N_LINE = 11, ATC_LDS_H_OFF_HTS = 12, ATC_LDS_H_SUB = 13, ATC_LDS_H_OFF_RESID = 14, ATC_LDS_H_N_RESID = 15,
       ATC_LDS_H_LDS_BYTES = 16, ATC_LDS_H_OFF_POOL = 17, ATC_LDS_H_N_REC = 18, ATC_LDS_HDR_WORDS = 24 };
enum { ATC_LDS_CLEAN = 0, ATC_LDS_LINE = 1, ATC_LDS_SUB = 2, ATC_LDS_RESID = 3 };

#define ATC_MAX_AIRCRAFT 64
#define ATC_OBS_DIM 10 /* atc_gym.py:262-277 */
#define ATC_ACT_DIM 3  /* v, h, phi  (atc_gym.py:70,79) */

/* per-aircraft flag word (outputs `flags`, 16 bits) */
enum {
    ATC_F_BELOW_MVA = 1u << 0, /* atc_gym.py:149-153 */
    ATC_F_OUTSIDE = 1u << 1,   /* atc_gym.py:156-161 */
    ATC_F_WON = 1u << 2,       /* atc_gym.py:163-169 */
    ATC_F_TIMEOUT = 1u << 3,   /* atc_gym.py:171-173 */
    ATC_F_INVALID_V = 1u << 4, /* atc_gym.py:312-315 via model.py:69-72 */
    ATC_F_INVALID_H = 1u << 5, /* atc_gym.py:312-315 via model.py:91-94 */
    ATC_F_CONFLICT = 1u << 6,  /* extension: 3 nm / 1000 ft separation lost (README.md:51) */
    ATC_F_NOISE = 1u << 7,     /* extension: inside a noise-abatement area below its ceiling (README.md:62) */
    ATC_F_INACTIVE = 1u << 8,  /* extension: aircraft already handed over (won earlier in this episode) */
    ATC_F_PHI_LIMIT = 1u << 9  /* the heading target of this step lay beyond +-2^52 counts (|a_phi| > 2.98e6) and was clamped there:
                                  the format's one remaining bound on the reference's unvalidated heading (model.py:104-120) */
};

/* params.mode bits */
enum {
    ATC_M_REWARD_SHAPING = 1u << 0,  /* SimParameters.reward_shaping, model.py:143 */
    ATC_M_NORMALIZE = 1u << 1,       /* SimParameters.normalize_state, model.py:144 */
    ATC_M_DISCRETE = 1u << 2,        /* SimParameters.discrete_action_space, model.py:145 */
    ATC_M_AUTO_RESET = 1u << 3,      /* VecEnv semantics: done envs are reset inside the step, obs := raw reset obs */
    ATC_M_RANDOM_ENTRY = 1u << 4,    /* reset draws (entry, level) from the counter-based RNG; else slot lattice */
    ATC_M_KEEP_ACTIVE = 1u << 5,     /* the reference's single-aircraft rule (atc_gym.py:163-169): an aircraft that reaches the
                                        corridor ends the episode and STAYS under control (no hand-over), so stepping on
                                        without reset keeps simulating it (learning/atc-gym-compute-performance.py:14-16) */
    ATC_M_ACTIONS_HELD = 1u << 6     /* atc_step only — a promise of the caller: `actions` holds, for every aircraft, the same
                                        bits as in the previous step of these envs — an atc_step or the last step of a multi-step launch (frame skip,
                                        learning/atc-gym-demo.py:18-19).  Results are identical to a launch without the bit;
                                        the kernel then skips the last_action record (16 of 118 bytes per aircraft-step):
                                        an aircraft under control in the previous step has last_action == its accepted
                                        targets (atc_gym.py:305-311), so no action is counted and the record does not
                                        change.  Envs reset since their last step (timesteps == 0) are handled in full.
                                        The previous step of an env that atc_branch wrote (child m*B + e) is the branch's step
                                        with actions[m]; of a child that was not evaluated (a byte copy), src env e's previous
                                        step; of an env that atc_state_select wrote, the previous step of the src env it was
                                        gathered from.
                                        Set on a launch whose actions DID change, actions_taken / last_action are wrong. */
};

typedef struct atc_params {
    double dt;              /* SimParameters.timestep [s], model.py:132-145 — a Python float in the reference: float64 here too
                               (ABI 20; 0.1 is not 0.1f), it scales every rate limit (model.py:75-78,97-100,117-120), the
                               displacement (model.py:126) and the base reward (atc_gym.py:137) */
    int32_t timestep_limit; /* 6000, atc_gym.py:40 */
    uint32_t mode;          /* ATC_M_* */
    uint64_t seed;          /* RNG key for ATC_M_RANDOM_ENTRY */
    float sep_nm;           /* 3.0  (extension) */
    float sep_ft;           /* 1000 (extension) */
    float conflict_reward;  /* -200 (extension) */
    uint32_t reserved0;     /* tag written into every chunk of atc_out_t.packet (ignored without a packet) */
    float reserved1;
    uint32_t reserved2;
} atc_params_t;

/* Aircraft positions (model.py:33-34) on the fp32 path.
 * The reference accumulates x, y in float64.  An fp32 accumulator drifts by up to half an ulp PER STEP on a straight leg
 * (1e-4 nm after 100 steps, measured) — beyond the 1e-5 bar.  Positions are therefore kept as 32-bit FIXED POINT on a
 * per-sector grid: nm = origin + fix * 2^-k, origin integer-valued, k the largest exponent (<= 27) whose range
 * +-2^(31-k) nm covers 1.5 x the sector's half extent (LOWW: origin (36, 42), k = 25: 3e-8 nm = 55 um steps, +-64 nm).
 *   - the per-step displacement (model.py:122-129; float64 from the fixed-point speed and heading, see below) advances the
 *     position by its value in counts rounded ONCE, saturating;
 *   - the fp32 position every formula of the reference sees is  (float)(origin + fix * 2^-k)  — ONE rounding (evaluated
 *     in float64, exact before the final conversion);
 *   - differences of positions are exact integers: the vector to the FAF (atc_gym.py:289-297) is
 *     (float)(faf_fix - fix) * 2^-k, the exact (33-bit, never saturating) difference rounded once — accurate to fp32 RELATIVE
 *     precision however close the aircraft is to the FAF, and as far from it as the grid reaches.
 * Accumulated rounding over a 6 000-step episode: <= 1.04e-6 nm measured against the float64 reference (dithered rounding, below);
 * half the bytes of a float64 pair.  The grid covers origin +- 2^(31-k) nm per axis (LOWW: +-64 nm around (36, 42), x in
 * [-28, 100), y in [-22, 106)).  An aircraft flown on without reset (the reference's FPS protocol,
 * learning/atc-gym-compute-performance.py) follows the reference up to that edge — within it, the vector to the FAF and with it
 * observation words 6-8 and the shaping reward too — and beyond it is pinned at the range limit (INT32_MIN / INT32_MAX counts):
 * from the step it crosses, the pinned x / y stop growing, and observation words 6-8 and the shaping reward, evaluated at the
 * pinned position, leave the reference's values, while the flags (it stays "outside the airspace" like the reference's, model.py:289), `done`, the time-out and the action counters stay
 * exact (tests/golden/g14: the protocol replayed for 10 000 steps per episode).
 *
 * Speed and heading (model.py:35-37, 60-129) on the fp32 path — ABI 18; unbounded heading: ABI 19.
 * The reference holds v, phi and the decoded action targets in float64.  As fp32 values they carry the rounding of the
 * target (1.5e-5 deg at 340 deg, 1.5e-5 kt at 250 kt) for as long as the target is held, and a heading that is 1e-5 deg off
 * moves the aircraft 5e-6 nm off over a 30 nm leg: next to the FAF, where the bearing to it is ill-conditioned, that was the one
 * stated exception to the 1e-5 bar of rounds 1-3 (tools/faf_conditioning.py).  Both are therefore 32-bit FIXED POINT, like
 * the positions, and the step's displacement is evaluated in float64 from them:
 *   speed    kt  = v_fix * 2^-23            UNSIGNED counts, [0, 512): the aircraft's [100, 300] and every refusable target
 *   heading  deg = 180 + P * 2^-23          signed counts P.  The reference never validates or wraps a heading (model.py:104-120:
 *                                           a continuous action a_phi = 3 turns the aircraft on to 720 deg), so P is NOT a 32-bit
 *                                           quantity: |P| <= 2^52 (+-5.4e8 deg).  What is STORED is two-level (ABI 19):
 *                                             phi_fix = sat32(P) in the 16-byte aircraft record — for -2^31 < P < 2^31 - 1, i.e.
 *                                               headings in (-76, 436) deg: the action space's [0, 360] and 76 deg either side,
 *                                               this IS the heading and nothing else is read or written;
 *                                             a record whose phi_fix is INT32_MIN / INT32_MAX is WIDE: its exact P is the
 *                                               integer-valued float64 atc_state_t.phi_wide[i][0] (written by the step that
 *                                               left the 32-bit range; float64 holds every integer up to 2^53).
 *                                           The last accepted heading target (last_action[2], atc_gym.py:311) is stored the same way:
 *                                           sat32 in last_act[i][1], exact value in phi_wide[i][1] when that is saturated.
 *   - a target is  counts = trunc(a * m + c):  ONE float64 fma on the fp32 action (m, c = the reference's factor / offset of
 *     atc_gym.py:64-78,318-335 in counts, both integers; exact for every fp32 action: 24 x 31 bits), truncated toward zero,
 *     NaN -> 0.  The speed's target is converted to uint32 SATURATING (gfx950: v_cvt_u32_f64): an action far outside the action
 *     space pins it at the end of the format's range, where it is refused like any target outside [100, 300] kt.  The heading's
 *     target is clamped to +-2^52 counts (|a_phi| <= 2.98e6 continuous, 5.4e8 discrete) — the one bound left: an aircraft-step
 *     whose heading target was clamped carries ATC_F_PHI_LIMIT; the aircraft still turns towards it at the rate limit, and all
 *     that differs from the reference is its action counter when two successive targets are BOTH beyond the bound and differ
 *     (tests/test_oracle_golden.py pins that step).
 *   - rate limits (model.py:75-78, 117-120) are exact integer arithmetic:  fix += clamp(target - fix, +-rint(rate dt 2^23))
 *     (wrapping 32-bit difference for the speed — speeds an Airplane can have, [100, 300] kt (model.py:22-23: the constructor
 *     raises outside), and the initial last_action 0 are < 2^31 counts apart; a speed placed from outside must lie inside
 *     [44, 356] kt, within 256 kt of every acceptable target: the host mirror's set_v refuses others —, exact for the heading: the 32-bit saturating
 *     form gives the same result whenever target and heading are both inside the 32-bit range, which is what the kernels
 *     evaluate for such lanes); the "action taken" discriminator (atc_gym.py:84,305-306) compares the same integer differences
 *     with 5 * 2^23 / 0.5 * 2^23 counts (targets are TRUNCATED to counts, each by less than one: two targets whose float64 difference is
 *     within a count — 1.2e-7 kt / deg — below the threshold can be exactly D counts apart and are then counted here and not by the
 *     reference; tests/golden/g15 holds such pairs);
 *   - what the heading feeds: the kinematics and every relative angle / the corridor window are periodic in the heading, the
 *     observation's raw heading (atc_gym.py:269) is not.  A heading inside the 32-bit range is used as it is:
 *       fp32 heading = fmaf((float)phi_fix, 2^-23, 180),  kinematics from phi_fix (below).
 *     A WIDE heading P is first wrapped, in float64 like the kinematics' own reduction:  Pw = fma(rint(P * ATC_PHI_INV_TURN),
 *       -ATC_PHI_TURN, P)  (exact: the remainder of P modulo 360 deg in counts, |Pw| <= 180 deg within a count):
 *       kinematics, relative angles and the corridor window use Pw exactly like a phi_fix;  observation word 3 is
 *       (float)(180 + P 2^-23) evaluated in float64 (exact) and rounded once — the float32 of the reference's float64 heading.
 *   - ONE angle decides a flag: the window of Corridor._inside_corridor_angle (model.py:212-231), `min_angle <= relative_angle <= 45`
 *     with min_angle = arccos(dir_rwy . dir_plane) in radians — in exact arithmetic 0 <= rel <= 45 deg.  Its relative angle is evaluated
 *     EXACTLY, on the counts:  rel = wrap(P - Q)  (wrap as above, float64 on integers), Q = rint((phi_to_runway - 180) 2^23);  the window
 *     holds for 0 < rel <= 45 * 2^23 and, for rel == 0, iff ATC_C_ALIGNED_OK (the reference's own rounding luck for an exactly aligned
 *     heading, evaluated on the host with its expression).  An fp32 heading could not decide it: an aircraft told to fly the runway
 *     heading holds it to within the fp32 rounding of its ACTION (340 -/+ 1e-5 deg), one third of an fp32 ulp at 340 — the reference's
 *     float64 tells the two apart, and so must the flag (tests/golden/g11: the winning intercepts flown at heading - 360).  The
 *     relative angles of the observation and the shaping terms are values (1e-5 bar) and stay fp32;
 *   - Vertical separation (extension: no reference code).  dh = |(float)h_a - (float)h_b|, the float32 difference of the altitudes
 *     rounded to float32 (what observation word 2 reports), in conflict iff dh < sep_ft and d^2 < sep_nm^2.  Levels a whole number of
 *     feet apart are exact in float32, so two aircraft levelled at commanded levels exactly sep_ft apart are not in conflict, whatever
 *     rounding noise their float64 altitudes carry (h + (target - h) need not equal target).  The float64 test oracle uses the same
 *     definition: with a float64 difference the verdict of such a pair hung on 3.6e-10 ft of noise.
 *   - Observation word 9 at the wrap.  relative_angle(phi_to_runway, phi) = (phi - phi_to_runway + 180) % 360 - 180 (atc_gym.py:284-287,
 *     model.py:340-342) is DISCONTINUOUS where the heading is the runway's reciprocal R: the reference returns -180 for phi == R and
 *     above, and +180 (the float32 of 179.99999999999997) for a heading a float64 rounding BELOW R — which its accumulated heading
 *     is whenever a turn in steps of 3 dt arrives at R with rounding noise (heading 159.99999999999997 for R = 160).  The float64
 *     oracle transcribes this as it is.  The fp32 spec evaluates the same formula on the fp32 heading fmaf(phi_fix, 2^-23, 180): every
 *     count within half an fp32 ulp of R (7.6e-6 deg at 160) reads -180, so word 9 — and the normalised word, by 2.0, its whole
 *     range — can sit on the other side of the wrap from the reference: where the reference's heading is a rounding below R while
 *     the counts are on it, and on every step of an aircraft that HOLDS R by a continuous action (the fp32 action, truncated, is one
 *     count below R: the reference reads +180, the spec -180).  -180 and +180 are the same angle; the shaping terms differ by less
 *     than 1e-8 there.  Tests compare word 9 modulo a turn inside 1e-3 deg of the wrap and count the rows (tests/helpers.py: obs_close;
 *     tests/ref_diff.py; pinned by tests/test_ref_diff.py).
 *   - the fp32 speed every other formula of the reference sees is (float)v_fix * 2^-23; both conversions are exact for every value
 *     with <= 24 significant bits, e.g. all integer speeds and headings;
 *   - the ALTITUDE (model.py:82-102) is the reference's float64, operation for operation (ABI 20; rounds 1-5 kept an fp32
 *     accumulator: exact for timesteps whose rate limits 41 dt / 15 dt are small multiples of an fp32 ulp — 1, 2, 5, 0.5 s — and
 *     0.4 ulp off PER STEP for 0.1 s: the below-MVA flag came one step late in 19 of 120 sustained descents, tests/golden/g12):
 *       target = a * m + c        one float64 fma on the fp32 action (the product is exact): the reference's a * f / 2 + f / 2 + off
 *                                 (atc_gym.py:333-335; discrete: a * 100 + 0, :329-330) bit for bit
 *       refused iff NOT (target >= h_min and target <= h_max)       (float64 compares; for every finite action the reference's
 *                                 `target < h_min or target > h_max`, model.py:91-94 — and a NaN target is refused, see below)
 *       h += max(min(target - h, 15 dt), -41 dt)       three float64 operations, dt the float64 of atc_params_t (model.py:95-102)
 *       below the MVA iff h < mva                       (atc_gym.py:149-153; the MVA height is an integer)
 *       observation words 2 and 5 = (float)h and (float)(h - mva), the difference in float64          (atc_gym.py:266,276)
 *     so every flag that depends on the altitude alone is the reference's for ANY timestep, including the ties it decides by its
 *     own accumulated rounding (15 000 ft - 3 000 x 4.1 ft against the 2 700 ft MVA at dt = 0.1).  What other formulas see — the
 *     glide-path test of the corridor (model.py:201-208), the shaping terms, the separation scan — is (float)h, one rounding.
 *     The last accepted altitude target (last_action[1], atc_gym.py:311) is kept as the same float64.
 *   - state placed from outside (entry points, fixtures) is the NEAREST count.
 *   - NON-FINITE ACTIONS.  A diverged policy emits NaN and +-Inf; the reference does not survive them, this library does.  No action
 *     value can put a NaN or an infinity into the state or into any output.  Per component (tests/test_action_edges.py, every value
 *     on every entry point; tests/golden/g15 pins the reference's side):
 *       speed     NaN -> 0 counts, refused (ATC_F_INVALID_V, -1, nothing applied, last_action kept).  +-Inf and +-FLT_MAX saturate at
 *                 the ends of the uint32 range and are refused like any target outside [100, 300] kt.
 *       altitude  NaN is REFUSED like a NaN speed (ATC_F_INVALID_H, -1, nothing applied, last_action kept): the refusal is written
 *                 `not (target >= h_min and target <= h_max)`.  +-Inf and +-FLT_MAX (6.5e42 ft as a float64) are outside the bounds
 *                 and refused.
 *       heading   never refused.  NaN -> 0 counts (180 deg), an ordinary target that is counted like one.  +-Inf and +-FLT_MAX are
 *                 clamped to +-2^52 counts with ATC_F_PHI_LIMIT; held, the clamped targets are EQUAL and counted once.
 *       +-0.0 and subnormal actions are ordinary numbers: the one rounding of the fma absorbs them.
 *     The reference, for comparison (nothing here follows it): its compares let a NaN target through (model.py:69-72, 91-94: `nan <
 *     v_min` is False), min / max pass it on and v, h or phi is NaN from then on — state, observation and reward stay NaN until
 *     reset, and every later step counts an action (`abs(nan - x) < d` is False, atc_gym.py:305).  An infinite speed or altitude
 *     target is refused, and the warning it prints, "%d" % inf (atc_gym.py:314), raises OverflowError out of step().  An infinite
 *     heading target turns the aircraft at the rate limit like here, but abs(inf - inf) is NaN, so the reference counts an action in
 *     EVERY step it is held where this library counts the first: that, like two different targets beyond +-2^52 above, is a
 *     difference of the action counter alone.
 *     (A change of results for actions no action space contains, with no record layout or signature touched: the ABI number stays,
 *     see ATC_ABI_VERSION.)
 * Heading kinematics (model.py:122-129, 345-348) in float64, shared bit for bit by every fp32 implementation (the HIP
 * kernels, the fp32 instantiation of the test oracle):
 *   k = rint(phi_fix * ATC_KIN_INV180)  [(180 * 2^23)^-1, nearest-even],  t = fma(k, -180 * 2^23, phi_fix)  (exact: the
 *   remainder in counts, |t| <= 90 * 2^23),  u = t * t,
 *   sin = t * (S0 + u (S1 + u (S2 + u (S3 + u (S4 + u S5))))),  cos = 1 + u (C1 + u (C2 + u (C3 + u (C4 + u C5))))
 *   (Horner, every step one fma; coefficients below: near-minimax in r = t pi / (180 * 2^23) on |r| <= pi/2, scaled to
 *   counts — tools/fit_kinematics_f64.py; max error 2.6e-11 / 4.4e-10);
 *   distance in position-grid counts  d = (double)v_fix * DA,  DA = ((double)dt / 3600) * 2^(k_pos - 23),  NEGATED when k is
 *   even (phi = 180 (1 + k) + t: an even k is an odd number of half turns);
 *   DITHERED ROUNDING:  x_fix += floor(sin * d + u11),  y_fix += floor(cos * d + u11)  (saturating adds), u11 = the low 11 bits of
 *   the env's time step (after its increment, atc_gym.py:135) bit-reversed, as a fraction in [0, 1) — the van der Corput
 *   sequence.  Plain rounding repeats the SAME round-off every step of a straight leg at constant speed (measured: up to
 *   7.8e-6 nm per episode); dithered, the round-offs of a constant displacement cancel to O(log n) counts over n steps.
 *   Evaluated as  r = fma(sin, d, M)  with M = the float64 whose high word is ATC_DITHER_MAGIC_HI (1.5 * 2^41) and whose low
 *   word is u11, i.e. M = 1.5 * 2^41 + u11 * 2^-11 (2^-11 is the last place of a float64 of that magnitude); the integer part of r is
 *   bits 11..42 of its pattern:  counts = (int32)(bits(r) >> 11).
 *   Requires 0.1423 dt 2^k_pos < 2^30 (512 kt: the displacement must fit 2^30 counts) and 5 dt < 256 (the speed's rate limit in
 *   counts): dt <= 51 s for any sector; atc_step refuses larger steps.
 * Measured against the float64 reference over the 650 963 steps of tests/golden/g9_wide.npz (tools/position_error.py):
 * positions within 1.5e-7 nm (median) / 1.04e-6 nm (maximum, 6 000-step episodes), speed and heading within one count;
 * the fixture replays at the plain 1e-5 bar everywhere — no near-FAF exception.
 *
 * Separation scan horizon (round 5; an implementation note, not a format: results are what a scan in every step gives).
 * Conflict = (d^2 < sep_nm^2) and (|dh| < sep_ft) for a pair of aircraft under control, d^2 = fma(dx, dx, dy dy) and dh from the
 * fp32 positions / altitudes.  The kinematics above bound what one step can do to a pair: an aircraft at or below 300 kt stays at or
 * below 300 kt (accepted speed targets lie in [100, 300] kt and the rate-limited move never overshoots) and moves by at most
 * (300 / 3600) dt nm (+ one position count per axis); its altitude moves by at most 15 dt ft up / 41 dt ft down (+ half an ulp).  A
 * pair with  d >= |sep_nm| + n (600 / 3600) dt  or  |dh| >= sep_ft + n 56 dt  (+ slack: 1e-5 relative + 1e-3 nm / 1 ft, hundreds of
 * times the fp32 evaluation error) therefore cannot be in conflict during the next n steps, whatever the actions.  Multi-step launches
 * (atc_rollout, atc_rollout_hold) of envs of more than 16 aircraft that do not report min_sep use this: a full scan notes which
 * groups of partners hold a pair inside those thresholds, and for the next n steps only those groups are scanned (none: no scan) —
 * unless an aircraft is above 300 kt or an altitude is beyond 2^17 ft in magnitude or NaN (then every step scans in full; no ACTION can
 * produce such an altitude any more — a NaN target is refused, see "NON-FINITE ACTIONS" — but state placed from outside still can, so the guard stays); an env
 * that is reset inside the launch ends the horizon of its wavefront.  tests/test_hip_edge_cases.py
 * (test_scan_horizon_on_the_fastest_closing_courses) drives pairs at exactly these closing rates through every phase of a horizon. */
#define ATC_V_FIX_SHIFT 23
#define ATC_PHI_FIX_SHIFT 23
#define ATC_PHI_FIX_OFFSET 180.0f
#define ATC_DITHER_MAGIC_HI 0x42880000u   /* high word of 1.5 * 2^41: the low word's low 11 bits are the dither fraction */
#define ATC_KIN_INV180 (0x1.6c16c16c16c17p-31)
#define ATC_KIN_HALF_TURN 1509949440.0    /* 180 * 2^23 */
#define ATC_PHI_TURN 3019898880.0         /* 360 * 2^23: a full turn in heading counts */
#define ATC_PHI_INV_TURN (0x1.6c16c16c16c17p-32)   /* RN(1 / ATC_PHI_TURN) */
#define ATC_PHI_LIMIT 4503599627370496.0  /* 2^52: heading targets are clamped to +-this (ATC_F_PHI_LIMIT) */
#define ATC_KIN_S0 (0x1.1df46a2514d5fp-29)
#define ATC_KIN_S1 (-0x1.dbb820c160971p-90)
#define ATC_KIN_S2 (0x1.dad945dddaa3dp-152)
#define ATC_KIN_S3 (-0x1.c366787a5df6bp-215)
#define ATC_KIN_S4 (0x1.f410ee5d4f8bep-279)
#define ATC_KIN_S5 (-0x1.5a91d219ad65ap-343)
#define ATC_KIN_C1 (-0x1.3f6a1d6c2409bp-59)
#define ATC_KIN_C2 (0x1.09b109e7441cbp-120)
#define ATC_KIN_C3 (-0x1.6198137ae3b3bp-183)
#define ATC_KIN_C4 (0x1.f762cae337122p-247)
#define ATC_KIN_C5 (-0x1.a6ebd88a524cfp-311)
#define ATC_POS_MAX_K 27

/* Persistent environment state (all device pointers).  Aircraft arrays are indexed env * N + k and packed so that a
 * wavefront moves each with one access per lane on consecutive addresses.  Per aircraft-step the step kernel reads
 * 16 + 8 + 12 B (record, altitude, action) and writes 16 + 8 B; the 16-byte last-action record is read and written only by
 * steps that may change it (not under ATC_M_ACTIONS_HELD, not inside a held block of a multi-step launch). */
typedef struct atc_state {
    int32_t* ac;      /* [B*N][4]  x_fix, y_fix (position grid counts, see above), phi_fix (heading, never wrapped, model.py:35-36;
                         fixed point, INT32_MIN / INT32_MAX = WIDE: see above and phi_wide), v_fix (speed, model.py:37; unsigned
                         counts) — one 16-byte record */
    double* alt;      /* [B*N]     altitude h [ft] (model.py:34): the reference's float64 (ABI 20, see "the ALTITUDE" above) */
    int32_t* last_act;/* [B*N][4]  last accepted v / phi / h targets = AtcGym.last_action (atc_gym.py:86,311) in the state's
                         own formats: word 0 v_fix, word 1 phi_fix (0 kt / 0 deg of atc_gym.py:86 = the counts of 0, not the
                         integer 0), words 2..3 the altitude target as a float64 — one 16-byte record */
    int32_t* env;     /* [B][ATC_ENV_WORDS]  per-step env record, see ATC_ENV_* */
    int32_t* stats;   /* [B][ATC_STAT_WORDS] per-episode env record, see ATC_STAT_* (touched only when an episode ends) */
    double* phi_wide; /* [B*N][4]  side record of aircraft whose 32-bit heading fields are saturated (see "Speed and heading": WIDE):
                         word 0 = exact heading counts, word 1 = exact last heading target (integer-valued float64, valid while
                         phi_fix / last_act[i][1] is INT32_MIN / INT32_MAX), word 2 = scratch of the step kernel (the wrapped
                         counts and observation word 3 of word 0, handed from the first half of a step to the second), word 3
                         reserved.  Never read or written for an aircraft whose heading and heading targets stay inside
                         (-76, 436) deg — every action inside the action space —, so it costs memory (32 B per aircraft), not
                         traffic; contents are unspecified while the 32-bit field is in range. */
} atc_state_t;
/* per-step env record (4 x 32-bit words; float fields are stored by bit pattern) */
enum {
    ATC_ENV_TIMESTEPS = 0,     /* i32  atc_gym.py:39 */
    ATC_ENV_ACTIONS_TAKEN = 1, /* i32  atc_gym.py:31 */
    ATC_ENV_TOTAL_REWARD = 2,  /* f32  atc_gym.py:30 */
    ATC_ENV_MASK_LO = 3,       /* u32  active mask bits 0..31: bit k = aircraft k still under control (extension) */
    ATC_ENV_WORDS = 4
};
/* per-episode env record (8 x 32-bit words) */
enum {
    ATC_STAT_EPISODES = 0,     /* i32  atc_gym.py:33 (_episodes_run) */
    ATC_STAT_EP_LENGTH = 1,    /* i32  length of the last finished episode (Monitor 'l') */
    ATC_STAT_EP_RETURN = 2,    /* f32  return of the last finished episode (Monitor 'r') */
    ATC_STAT_WIN_BITS = 3,     /* u32  last 10 episode outcomes, bit0 = most recent (atc_gym.py:36-37,359-363) */
    ATC_STAT_EP_ACTIONS = 4,   /* i32  actions_taken of the last finished episode: actions_per_timestep (atc_gym.py:197)
                                       keeps its last value across reset() = EP_ACTIONS / EP_LENGTH */
    ATC_STAT_MASK_HI = 5,      /* u32  active mask bits 32..63 (read / written per step only by envs of more than 32 aircraft) */
    ATC_STAT_WORDS = 8
};

/* Per-step outputs (device pointers; nullable ones may be NULL). */
typedef struct atc_out {
    float* obs;        /* [B*N*10] what step() returns (normalised iff ATC_M_NORMALIZE), atc_gym.py:187-192 */
    float* raw_obs;    /* nullable [B*N*10] info["original_state"], atc_gym.py:192 */
    float* reward;     /* [B] env reward = sum over aircraft */
    float* ac_reward;  /* nullable [B*N] per-aircraft reward */
    uint8_t* done;     /* [B] */
    uint16_t* flags;   /* [B*N] ATC_F_* */
    float* min_sep;    /* nullable [B] minimum horizontal separation among active pairs [nm] (diagnostic) */
    float* term_obs;   /* nullable [B*N*10] terminal observation of envs that were auto-reset this step */
    uint32_t* packet;  /* nullable, N == 1 only: [B][ATC_PKT_CHUNKS][4] — the step result of one env as self-validating
                          16-byte chunks, for a host that polls pinned mapped memory instead of synchronising the stream
                          (the single-env AtcGym).  Every chunk = 3 payload words + params.reserved0 (the caller's step
                          sequence number) and is written with ONE 16-byte store, so a reader that sees the expected tag in
                          a chunk and THEN reads its payload has that step's values whatever order the chunks arrive in:
                          obs[10], raw obs[10], reward | flags + (done << 16), timesteps, actions_taken | x, y grid counts */
} atc_out_t;
#define ATC_PKT_CHUNKS 9

/* Opaque device-resident scenario (owned by the library). */
typedef struct atc_scenario atc_scenario_t;

/* -- lifecycle -------------------------------------------------------------------------------- */
int atc_abi_version(void);
const char* atc_last_error(void);

/* Launch record (ABI 22).  The step kernel is one template compiled once per lane-group width W (1, 2, 4, ..., 64: the aircraft
 * count rounded up to a power of two) and FORM; the library picks one per launch from B, N, T, the optional outputs, the device's
 * CU count and whether an LDS table is attached.  Every thread counts its own launches: slot = log2(W) * ATC_LF_FORMS + form for
 * the step kernel, ATC_LAUNCH_SERVE for starts of the step server.  Host side only — nothing that is launched depends on it. */
enum {
    ATC_LF_FULL_ONE = 0,    /* T = 1, an optional output or a packet requested */
    ATC_LF_FULL_MULTI = 1,  /* T > 1, an optional output requested */
    ATC_LF_GEN_ONE = 2,     /* T = 1, required outputs only, idle lanes possible */
    ATC_LF_ALLV_ONE = 3,    /* T = 1, required outputs only, N == W and B * W a multiple of 256: every lane is an aircraft */
    ATC_LF_GEN_MULTI = 4,   /* T > 1, required outputs only, idle lanes possible */
    ATC_LF_ALLV_MULTI = 5,  /* T > 1, every lane an aircraft, more than 2 wavefronts per SIMD of the device */
    ATC_LF_LAT = 6,         /* T > 1, every lane an aircraft, at most 2 wavefronts per SIMD (8 per CU) */
    ATC_LF_LDSG = 7,        /* LAT with W = 1, an LDS table attached and B <= 256 * CUs (exists for W = 1 only) */
    ATC_LF_FORMS = 8,
    ATC_LAUNCH_SERVE = 56,  /* atc_serve_start */
    ATC_LAUNCH_SLOTS = 57
};
/* Copies the calling thread's first min(n, ATC_LAUNCH_SLOTS) counters to out (launches since the thread started; they only grow,
 * a failed launch is not counted).  atc_step_multi and atc_step_packet count once per launch they make. */
int atc_launch_counts(uint64_t* out, int n);
/* The frame-skip kernel (atc_step_skip) keeps a record of its own, so that the one above stays as it is: slot = log2(W), one per
 * lane-group width.  Same rules: per calling thread, only grows, a refused or failed call is not counted. */
enum {
    ATC_SKIP_MAX = 255,          /* largest frame-skip length K (n_steps is a byte) */
    ATC_SKIP_LAUNCH_SLOTS = 7
};
int atc_skip_launch_counts(uint64_t* out, int n);
/* Fill-phase prefetch of the fast single-step launch (required outputs only, N a power of two <= 16, B * N a multiple of 256): the
 * workgroups the first `resident` hold at once also request the state and action lines of the workgroup `resident` further on,
 * into the L2 that workgroup will read them from.  Results do not depend on it.  *resident = the device's resident workgroups for
 * that kernel (the runtime's occupancy x CUs, rounded down to a multiple of 8; 0 where the form does not apply), *stride = what an
 * atc_step of B x N passes to the kernel: `resident` when the launch has more workgroups (B * N / 256) than that, else 0 (off) —
 * and 0 always with ATC_NO_FILL_PREFETCH set in the environment (developer knob, read once per process).  With a residency cap
 * (ATC_STEP_RESIDENT=<k> in the environment, developer knob, read once per process; the library ships none) `resident` is the
 * capped figure, k x CUs rounded down likewise, which is also the stride such a launch uses.  Host side only. */
int atc_fill_prefetch_info(const atc_scenario_t* s, int B, int N, int* resident, int* stride);

/* Uploads a compiled scenario blob (host pointer, n_words floats) to `device`.
 * Replaces: AtcGym.__init__ scenario unpacking, atc_gym.py:45-58. */
int atc_scenario_create(const float* blob_host, size_t n_words, int device, atc_scenario_t** out);
int atc_scenario_destroy(atc_scenario_t* s);
/* Attaches (copies to the device) an LDS-resident lookup table — see "LDS-resident lookup table" above — or detaches the current
 * one (table_host == NULL).  Every code and offset is validated here; -1 if the table is malformed, larger than the device's LDS
 * per workgroup, or the scenario has no lookup grid / has noise-abatement areas.  With a table attached, atc_rollout[_hold] of
 * one-aircraft envs with at most 256 envs per CU of the device (65 536 on MI355X) stage it in LDS; every other launch ignores it.
 * Not thread-safe against launches that use the same handle concurrently (attach before stepping). */
int atc_scenario_attach_lds_table(atc_scenario_t* s, const void* table_host, size_t n_bytes);

/* Zero-copy for latency-bound callers (the single-env AtcGym, atc_gym.py:128-192, whose step is one aircraft): every
 * state / action / output pointer may also address pinned host memory (hipHostMalloc, e.g. a torch tensor with
 * pin_memory()) that is mapped into the device's address space; the kernels then read and write it over the host link
 * and no copy is launched around the step.  *dev receives the device address of such a buffer; fails (-2) if `host`
 * is not mapped pinned memory. */
int atc_host_mapped_ptr(const void* host, void** dev);

/* -- batched queries (same device functions as the step kernel) -------------------------------- */
/* Airspace.get_mva_height, model.py:282-292.  out_h[i] = MVA height [ft] or -1 (outside airspace).
 * use_grid != 0 uses the lookup grid if the blob has one. */
int atc_query_mva(const atc_scenario_t* s, int n, const float* x, const float* y, int32_t* out_h, int use_grid,
                  void* stream);
/* Airspace.find_mva, model.py:282-289: out_idx[i] = index of the MVA polygon in list order, or -1. */
int atc_query_mva_index(const atc_scenario_t* s, int n, const float* x, const float* y, int32_t* out_idx, int use_grid,
                        void* stream);
/* Airspace.get_mva_height through the attached LDS table (diagnostic / test entry): out_h as atc_query_mva; from_lds[i] (may be
 * NULL) = 1 where the table answered, 0 where the point's wavefront (64 consecutive points) went to the lookup grid. */
int atc_query_mva_lds(const atc_scenario_t* s, int n, const float* x, const float* y, int32_t* out_h, uint8_t* from_lds,
                      void* stream);
/* Runway.inside_corridor, model.py:248-257,188-231.  angle_only != 0 evaluates Corridor._inside_corridor_angle
 * (model.py:212-231) alone.  out[i] = 0/1. */
int atc_query_corridor(const atc_scenario_t* s, int n, const float* x, const float* y, const float* h,
                       const float* phi, int angle_only, uint8_t* out, void* stream);
/* Shaping rewards, atc_gym.py:199-260: out3[3*i+0..2] = (_reward_approach_position, _reward_approach_angle,
 * _reward_glideslope) for inputs (d_faf, phi_rel_faf, phi_plane, h, on_gp_altitude). */
int atc_query_shaping(const atc_scenario_t* s, int n, const float* d_faf, const float* phi_rel_faf,
                      const float* phi_plane, const float* h, const float* on_gp, float* out3, void* stream);

/* -- environment ------------------------------------------------------------------------------- */
/* AtcGym.reset, atc_gym.py:337-365, for every env whose mask byte is non-zero (mask == NULL: all envs).
 * Writes the RAW reset observation (mva = 0, quirk atc_gym.py:351,365) to `obs` for reset envs only.
 * first != 0 additionally clears the last-action fields / win_bits / episodes (what AtcGym.__init__ does,
 * atc_gym.py:29-41,86). */
int atc_reset(const atc_scenario_t* s, int B, int N, const atc_state_t* st, const uint8_t* mask, float* obs,
              const atc_params_t* p, int first, void* stream);

/* AtcGym._get_state(0), atc_gym.py:262-277,351: RAW observation (mva = 0) of the CURRENT aircraft state of every masked
 * env (mask == NULL: all) — used after the host places aircraft explicitly (e.g. to replay the reference's
 * random.choice entry draws, atc_gym.py:346-348). */
int atc_observe(const atc_scenario_t* s, int B, int N, const atc_state_t* st, const uint8_t* mask, float* obs,
                const atc_params_t* p, void* stream);

/* AtcGym.step, atc_gym.py:128-192, for B envs x N aircraft.  actions: [B*N*3] (v,h,phi per aircraft),
 * continuous in [-1,1] or discrete indices stored as floats (atc_gym.py:318-335). */
int atc_step(const atc_scenario_t* s, int B, int N, const atc_state_t* st, const float* actions,
             const atc_out_t* out, const atc_params_t* p, void* stream);

/* One step of several INDEPENDENT sub-batches with a single call — the arguments of n atc_step calls, each with its own
 * state, outputs and (normally) its own stream.  Meant for pipelined callers that keep a few sub-batches in flight on
 * separate streams with no join between steps: the launch ramp and tail of one sub-batch then overlap the body of the
 * others (65 536 x 16 as 2-4 sub-batches: 21.6-23.4 us per step of all envs instead of 24.9 us), and the host pays one
 * foreign call per step instead of n.  Stops at the first failing launch and returns its error. */
typedef struct atc_step_call {
    const atc_scenario_t* s;
    int32_t B, N;
    const atc_state_t* st;
    const float* actions;
    const atc_out_t* out;
    const atc_params_t* p;
    void* stream;
} atc_step_call_t;
int atc_step_multi(int n, const atc_step_call_t* calls);

/* atc_step of ONE env x ONE aircraft (B = N = 1) whose outputs include out->packet in pinned mapped memory, followed by the
 * wait for its result in the same foreign call.  `actions` is a HOST pointer to the 3 action values here: they are read
 * during the call and travel with the kernel arguments (no read over the host link on the device side).
 * The step is launched with p->reserved0 = seq, then `packet_host` (the HOST
 * address of the same packet buffer) is polled until all ATC_PKT_CHUNKS chunks carry the tag `seq`, and their 27 payload
 * words are copied to payload[27] (see atc_out_t.packet for their meaning).  Returns 0, the launch's error, or -3 when the
 * result has not arrived within `timeout_us` microseconds (the caller then synchronises the stream and reads the packet itself).
 * `seq` must differ from the previous call's; `packet_host` must be 16-byte aligned (each chunk is read with one 16-byte load, so
 * a tag and the payload words it validates always come from the same access).  The kernel's trailing state stores may still be in flight on return: anything
 * else that touches the env's buffers has to drain the stream first.  Replaces the wait in AtcGym.step (atc_gym.py:128-192). */
int atc_step_packet(const atc_scenario_t* s, const atc_state_t* st, const float* actions, const atc_out_t* out,
                    atc_params_t* p, uint32_t seq, const uint32_t* packet_host, uint32_t* payload, int timeout_us, void* stream);

/* Persistent step server for ONE env x ONE aircraft (ABI 20) — what the drop-in AtcGym steps through (atc_gym.py:128-192; the
 * reference's callers step one env per process: learning/atc-gym-stable-baselines.py:69-80, atc-gym-compute-performance.py:10-19).
 * atc_serve_start launches ONE resident wavefront that keeps the env's state in registers and polls `mailbox` — 64 bytes of pinned
 * mapped host memory (hipHostMalloc / a pinned torch tensor), 64-byte aligned — for commands; atc_serve_step writes {3 action
 * floats, seq} into it with one 16-byte store and polls out->packet (see atc_out_t.packet; `packet_host` / `payload` as in
 * atc_step_packet) for the 9 chunks tagged `seq`; no kernel launch, argument upload or state round trip per step.
 *   mailbox words: 0..2 action (float bits), 3 sequence number (0xffffffff = quit) — written by the host;
 *                  4 server state (0 not yet running, 1 serving, 2 left: lease ran out, 3 left: quit), 5 last served sequence
 *                  number — written by the device.
 *   - `seq` of atc_serve_start = the sequence number of the LAST step already taken (the first atc_serve_step uses seq + 1, every
 *     further one the previous + 1); 0xffffffff is reserved.
 *   - the server leaves by itself after `lease_us` microseconds (>= 10) without a command: atc_serve_step then returns -4 for the
 *     command it did not see and the caller starts the server again (same seq rule) and repeats the call.  -3: no answer within
 *     `timeout_us` (the caller falls back to atc_serve_stop + atc_step_packet).
 *   - CHOOSING THE LEASE.  A resident kernel occupies a hardware queue; a process has few (4 by default) and HIP streams beyond that
 *     share them: work submitted to a stream that shares the server's queue waits until the server has left.  A caller that steps
 *     in a tight loop and submits nothing else (the reference's FPS script) can use any lease; a caller that interleaves other GPU
 *     work keeps it at the scale of a kernel launch — envs.atc.atc_gym.AtcGym uses 50 us and only serves while its steps follow
 *     each other within 50 us (otherwise it steps by atc_step_packet): the worst a colliding stream can wait is one lease.
 *   - WHILE THE SERVER RUNS the env's state lives in its registers: nothing else may read or write the env's atc_state_t buffers or
 *     launch on `stream` (a launch would queue behind the resident kernel).  atc_serve_stop sends quit and synchronises the stream:
 *     after it the state is in memory as after an atc_step.  Outputs other than the packet (obs, reward, ...) are written every step
 *     like atc_step's.
 * Results are those of atc_step on the same state and actions, bit for bit (same device functions). */
int atc_serve_start(const atc_scenario_t* s, const atc_state_t* st, const atc_out_t* out, const atc_params_t* p,
                    uint32_t* mailbox_host, uint32_t seq, int lease_us, void* stream);
int atc_serve_step(uint32_t* mailbox_host, const float* actions, uint32_t seq, const uint32_t* packet_host, uint32_t* payload,
                   int timeout_us);
int atc_serve_stop(uint32_t* mailbox_host, void* stream);

/* T consecutive steps in ONE launch with aircraft state held in registers.  actions: [T][B*N*3];
 * outputs are [T][...] versions of atc_out_t (each pointer strides by its per-step size).
 * Requires ATC_M_AUTO_RESET semantics to be meaningful for T > episode length. */
int atc_rollout(const atc_scenario_t* s, int B, int N, int T, const atc_state_t* st, const float* actions,
                const atc_out_t* out, const atc_params_t* p, void* stream);

/* The same with every action HELD for `hold` consecutive steps (frame skip — the protocol of the reference's demo loop,
 * learning/atc-gym-demo.py:18-19: one sampled action is applied 20 times): actions: [T / hold][B*N*3], step t uses
 * block t / hold; T must be a multiple of hold (ATC_ERR_ARG otherwise: a partial last block is refused, not read).
 * Results are identical to atc_rollout with each block repeated `hold` times; the action tensor and its
 * HBM traffic shrink by that factor. */
int atc_rollout_hold(const atc_scenario_t* s, int B, int N, int T, int hold, const atc_state_t* st, const float* actions,
                     const atc_out_t* out, const atc_params_t* p, void* stream);

/* FRAME SKIP: one decision, up to K steps, ONE transition — the loop of the reference's demo (learning/atc-gym-demo.py:14-22: a
 * sampled action is applied for 20 steps) as a vectorised env's `frame_skip` knob.  1 <= K <= ATC_SKIP_MAX.  Defined per env as
 *
 *     n = 0
 *     repeat: atc_step the env once with `actions` (the same [N][3] block every time); n += 1
 *     until that step reported done, or n == K
 *
 * and everything returned or left behind follows from the atc_step results of the n executed steps, in step order:
 *   obs, raw_obs      those of the LAST executed step (under ATC_M_AUTO_RESET and done: the raw reset observation, exactly as
 *                     atc_step returns it in that step)
 *   reward, ac_reward float32 sum of the executed steps' values, accumulated sequentially in step order (acc = r1; acc = acc + r2;
 *                     ... — plain float32 additions, never fused: reproducible bit for bit by a host loop over atc_step)
 *   done              1 iff the last executed step reported done
 *   flags             bitwise OR of the executed steps' flag words
 *   min_sep           minimum over the executed steps
 *   term_obs          as atc_step writes it in the terminating step (envs auto-reset in this call); untouched otherwise
 *   n_steps           [B] bytes (may be NULL): n
 *   out->packet       must be NULL
 * STATE afterwards (all of atc_state_t, the per-episode record included) is bit for bit what n atc_step calls leave: an env that
 * ended at step n < K is NOT stepped again in this call — a transition never spans two episodes.  Without ATC_M_AUTO_RESET it sits
 * in its terminal state, with it in its fresh spawn state with timesteps == 0.  The last-action record and actions_taken behave as
 * n single steps with the same actions do: the first step may count actions, the repeats cannot.  Envs are independent: an env's
 * result does not depend on whether its neighbours stopped early.  K == 1 is atc_step, outputs and state, bit for bit.
 * ATC_ERR_ARG (atc_last_error() says which): K outside 1 .. 255 — checked first, before any pointer —, the argument errors of
 * atc_step, out->packet != NULL, ATC_M_ACTIONS_HELD in p->mode (that bit is atc_step's; the first step of a skip call always
 * carries a fresh decision).
 * One launch: the state is read and written once and one set of outputs is stored, where K atc_step calls stream both K times and
 * atc_rollout_hold(T = K, hold = K) stores [K][...] outputs and steps THROUGH resets.  Counted by atc_skip_launch_counts only. */
int atc_step_skip(const atc_scenario_t* s, int B, int N, int K, const atc_state_t* st, const float* actions /* [B*N*3] */,
                  const atc_out_t* out, uint8_t* n_steps /* nullable [B] */, const atc_params_t* p, void* stream);

/* TRAFFIC OBSERVATION (extension): what each aircraft sees of the others.  The ten observation words per aircraft (ATC_OBS_DIM,
 * atc_gym.py:262-277) say nothing about any other aircraft, although envs of N > 1 aircraft carry the separation scan and its
 * penalty.  atc_observe_traffic is a query of the CURRENT state — a launch of its own, separate from the step: for every aircraft
 * the K nearest other aircraft under control in the same env, nearest first, each as a record of ATC_TRAFFIC_DIM words in the
 * observing aircraft's own frame.  1 <= K <= ATC_TRAFFIC_MAX_K.
 *
 * Reads st->ac, st->alt, the active mask (ATC_ENV_MASK_LO, and ATC_STAT_MASK_HI for N > 32) and st->phi_wide (only for aircraft
 * whose phi_fix is saturated); writes nothing but `traffic`: the state is bit-identical afterwards.
 *
 * Candidates and order.  For aircraft i of env e the candidates are the slots j != i of that env whose active-mask bit is set.
 * With the fp32 positions every other formula sees (pos_to_real = (float)(origin + fix 2^-k), one rounding):
 *     dx = xj - xi,  dy = yj - yi,  d2 = fma(dx, dx, dy * dy)          (the separation scan's own expression)
 * Candidates are ordered by (d2, j) ascending — exact ties go to the lower slot; d2 is finite and non-negative, so its bit pattern
 * orders it and the order is an integer result: exact.  Record r < min(K, candidates) describes the r-th candidate; the remaining
 * records are ABSENT: words 0..6 = 0, word 7 = -1.  An aircraft that is itself not under control (mask bit clear) gets K absent
 * records; so does every aircraft of a one-aircraft env.
 *
 * A present record (fp32 operations, each rounded once, unless stated):
 *   ATC_T_PRESENT   1
 *   ATC_T_DIST      sqrt(d2) [nm]
 *   ATC_T_AHEAD     dx sin(th) + dy cos(th)          th = aircraft i's heading, a compass heading (model.py:122-129): "ahead" is
 *   ATC_T_RIGHT     dx cos(th) - dy sin(th)          (sin th, cos th), "right" is (cos th, -sin th).  th comes from the heading
 *                                                    counts (a WIDE heading wrapped first, as atc_observe does); sin / cos by the
 *                                                    kinematics' float64 polynomials or any evaluation accurate to 1e-6
 *   ATC_T_DH        (float)hj - (float)hi [ft]       the scan's expression without the absolute value: exact
 *   ATC_T_DV_AHEAD  the relative ground velocity dv = vel_j - vel_i [kt], vel = v (sin phi, cos phi), v = v_fix 2^-23, rotated into
 *   ATC_T_DV_RIGHT  i's frame exactly like (dx, dy).  An intruder ahead with a negative ATC_T_DV_AHEAD is closing.
 *   ATC_T_SLOT      (float)j
 * With ATC_M_NORMALIZE in p->mode words 1..3 are divided by ATC_C_WORLD_DIAG, word 4 by ATC_C_H_MAX, words 5..6 by 2 ATC_C_V_MAX
 * (word 4 as the correctly rounded fp32 quotient — it is exact before; the others as a product with the fp32 reciprocal, they are
 * values); words 0 and 7 are never scaled.
 *
 * ATC_ERR_ARG: K outside 1 .. 8 — checked first, before any pointer —, traffic == NULL, the argument errors of atc_observe.
 * Counted by atc_traffic_launch_counts only: slot = log2(W), per calling thread, only grows, a refused or failed call is not
 * counted (the rules of atc_skip_launch_counts). */
#define ATC_TRAFFIC_DIM 8
#define ATC_TRAFFIC_MAX_K 8
enum { ATC_T_PRESENT = 0, ATC_T_DIST = 1, ATC_T_AHEAD = 2, ATC_T_RIGHT = 3, ATC_T_DH = 4,
       ATC_T_DV_AHEAD = 5, ATC_T_DV_RIGHT = 6, ATC_T_SLOT = 7 };
int atc_observe_traffic(const atc_scenario_t* s, int B, int N, int K, const atc_state_t* st,
                        float* traffic /* [B*N][K][ATC_TRAFFIC_DIM] */, const atc_params_t* p, void* stream);
enum { ATC_TRAFFIC_LAUNCH_SLOTS = 7 };
int atc_traffic_launch_counts(uint64_t* out, int n);

/* WHAT-IF LOOK-AHEAD (extension): "from the state this env is in now, what happens if I hold decision m for K steps?" for M candidate
 * action blocks per env in ONE launch that never writes state — the primitive behind MPC / CEM action selection, action shields and
 * tree-search rollouts.  1 <= K <= ATC_SKIP_MAX, 1 <= M <= ATC_LOOKAHEAD_MAX_M.  Defined per candidate m and env e as
 *
 *     atc_step_skip(s, B, N, K, <a bit-exact private copy of the env's state>, actions[m], ..., p, stream)
 *
 * i.e. the env steps with actions[m] (the same [N][3] block every time) until a step reports done or n == K, exactly as there:
 *   reward, ac_reward [m] float32 sum of the executed steps' values, accumulated sequentially in step order
 *   flags [m]         bitwise OR of the executed steps' flag words
 *   min_sep [m]       minimum over the executed steps
 *   done [m]          1 iff the last executed step reported done
 *   n_steps [m]       n, the number of executed steps
 *   obs [m]           that of the last executed step (under ATC_M_AUTO_RESET and done: the raw reset observation, drawn with the
 *                     episode number the copy would have used)
 * Candidates are independent: candidate m's result does not depend on M, on the other candidates or on neighbouring envs; M == 1
 * with every output requested reproduces atc_step_skip's corresponding outputs bit for bit.  reward and done are required, every
 * other output pointer may be NULL; a launch that asks for none of flags, ac_reward, min_sep, obs runs a form with them compiled out.
 * STATE: the call reads atc_state_t and writes none of it — all six arrays are byte-identical afterwards, `stats` (no per-episode
 * record update on a look-ahead reset) and `phi_wide` (the step's scratch word 2 included).  There is no term_obs.
 * LIMIT — WIDE headings (ABI 19).  The step hands a WIDE heading from step to step through the phi_wide side record in memory, which
 * this call may not write.  An env-candidate is therefore NOT EVALUATED when any aircraft's heading or accepted heading target is
 * WIDE at the start (phi_fix or last_act[.][1] saturated) or becomes WIDE during the K steps: n_steps = 0, done = 0, reward = 0 and
 * every requested per-aircraft / per-env output word of that (m, e) is 0.  Other candidates of the env are unaffected.  Every action
 * inside the action space keeps headings within (-76, 436) deg: only callers that feed out-of-range heading actions meet this.
 * ATC_ERR_ARG, in this order, the first two before any pointer is looked at: K outside 1 .. ATC_SKIP_MAX; M outside 1 ..
 * ATC_LOOKAHEAD_MAX_M; out, out->reward or out->done NULL; the argument errors of atc_step; ATC_M_ACTIONS_HELD in p->mode.
 * Counted by atc_lookahead_launch_counts only (slot = log2(W); the rules of atc_skip_launch_counts): atc_launch_counts and
 * atc_skip_launch_counts do not move. */
#define ATC_LOOKAHEAD_MAX_M 64
typedef struct atc_lookahead_out {
    float*    reward;    /* [M][B]      required */
    uint8_t*  done;      /* [M][B]      required */
    uint8_t*  n_steps;   /* [M][B]      nullable; 0 = not evaluated (see WIDE above) */
    uint16_t* flags;     /* [M][B*N]    nullable */
    float*    ac_reward; /* [M][B*N]    nullable */
    float*    min_sep;   /* [M][B]      nullable */
    float*    obs;       /* [M][B*N*10] nullable */
} atc_lookahead_out_t;
int atc_lookahead(const atc_scenario_t* s, int B, int N, int K, int M, const atc_state_t* st, const float* actions /* [M][B*N*3] */,
                  const atc_lookahead_out_t* out, const atc_params_t* p, void* stream);
enum { ATC_LOOKAHEAD_LAUNCH_SLOTS = 7 };
int atc_lookahead_launch_counts(uint64_t* out, int n);
/* Developer knob (A/B runs, tests): how the candidates map onto the launch, for the calling thread's later atc_lookahead calls.
 * n = 1: one workgroup per (256-slot tile, candidate); n = M or more: one workgroup per tile that loops over all candidates; in
 * between: n candidates per workgroup; 0: the library's choice (the default).  Results do not depend on it.  ATC_ERR_ARG outside
 * 0 .. ATC_LOOKAHEAD_MAX_M. */
int atc_lookahead_set_mapping(int candidates_per_workgroup);

/* PLAN LOOK-AHEAD (extension): atc_lookahead for candidates that are SEQUENCES — M plans per env, each H action blocks held for K
 * steps one after the other ("turn now, descend in 20 s, slow down after that"), scored in ONE launch that never writes state: what
 * CEM / MPPI sample and weight by a discount.  1 <= K <= ATC_SKIP_MAX, 1 <= H <= ATC_PLAN_MAX_H, 1 <= M <= ATC_LOOKAHEAD_MAX_M.
 * Defined per candidate m and env e, on a bit-exact private copy of the env's state, as
 *
 *     n = 0
 *     for h = 0 .. H-1:
 *         r_h = atc_step_skip(copy, K, actions[m][h])      everything atc_step_skip defines
 *         n += r_h.n_steps
 *         if r_h.done: break                               a plan never spans two episodes, ATC_M_AUTO_RESET or not
 *
 *   seg_reward [m][h]  r_h.reward for an executed segment, 0 for a segment after the break
 *   reward [m]         the float32 sum of the executed segments' r_h.reward, accumulated sequentially in segment order
 *                      (acc = r_0; acc = acc + r_1; ...; plain additions, never fused): a host loop over atc_step_skip outputs
 *                      reproduces it bit for bit
 *   ac_reward [m]      the same two-level sum per aircraft
 *   flags [m]          bitwise OR over all executed steps
 *   min_sep [m]        minimum over all executed steps
 *   done [m]           the last executed segment's done
 *   obs [m]            the last executed segment's obs (after a look-ahead reset under ATC_M_AUTO_RESET: the raw reset observation,
 *                      as atc_lookahead defines it)
 *   n_steps [m]        n, the total of executed steps (<= H K = 4080); the number of executed segments is ceil(n / K)
 * The first step of every segment carries a fresh decision: the last-action record, actions_taken and the refused-target verdict
 * behave as the chain above makes them (carried inside the launch, never stored).
 * Candidates are independent of each other, of M and of neighbouring envs.  H == 1 reproduces atc_lookahead bit for bit in every
 * shared output (n_steps carries the same values).  The first h segments of a plan give the seg_reward of a call with H = h on the
 * plan's prefix.  reward and done are required, every other output pointer may be NULL; a launch that asks for none of flags,
 * ac_reward, min_sep, obs runs a form with them compiled out (seg_reward and n_steps are available in both forms).
 * STATE: the call reads atc_state_t and writes none of it — all six arrays are byte-identical afterwards, `stats` and the phi_wide
 * scratch word included.
 * LIMIT — WIDE headings: atc_lookahead's rule over all segments.  An env-candidate is NOT EVALUATED when any aircraft's heading or
 * accepted heading target is WIDE at the start or becomes WIDE in any executed step of any segment: n_steps = 0, done = 0, reward = 0
 * and every requested word of that (m, e) is 0 — the seg_reward of segments already run included.
 * ATC_ERR_ARG, in this order, the first three before any pointer is looked at: K outside 1 .. ATC_SKIP_MAX; H outside 1 ..
 * ATC_PLAN_MAX_H; M outside 1 .. ATC_LOOKAHEAD_MAX_M; out, out->reward or out->done NULL; the argument errors of atc_step;
 * ATC_M_ACTIONS_HELD in p->mode.
 * Counted by atc_plan_launch_counts only (slot = log2(W); the rules of atc_skip_launch_counts): the other launch records do not move.
 * atc_lookahead_set_mapping governs this call's candidates per workgroup as well. */
#define ATC_PLAN_MAX_H 16
typedef struct atc_plan_out {
    float*    reward;     /* [M][B]      required */
    uint8_t*  done;       /* [M][B]      required */
    uint16_t* n_steps;    /* [M][B]      nullable; total executed steps (<= H*K = 4080); 0 = not evaluated */
    float*    seg_reward; /* [M][H][B]   nullable */
    uint16_t* flags;      /* [M][B*N]    nullable */
    float*    ac_reward;  /* [M][B*N]    nullable */
    float*    min_sep;    /* [M][B]      nullable */
    float*    obs;        /* [M][B*N*10] nullable */
} atc_plan_out_t;
int atc_lookahead_plan(const atc_scenario_t* s, int B, int N, int K, int H, int M, const atc_state_t* st,
                       const float* actions /* [M][H][B*N*3] */, const atc_plan_out_t* out, const atc_params_t* p, void* stream);
enum { ATC_PLAN_LAUNCH_SLOTS = 7 };
int atc_plan_launch_counts(uint64_t* out, int n);

/* DRAWN PLANS (extension): atc_lookahead_plan whose M candidates are DRAWN inside the launch from a mean, a standard deviation and a
 * counter-based key, so that a sampling planner (CEM, MPPI) never builds the [M][H][B*N*3] candidate tensor: M H B N 12 bytes that are
 * written, read once and thrown away.  The few plans a caller needs afterwards (the elites, the winner) are regenerated exactly from
 * their candidate numbers by atc_plan_draw.  1 <= M <= ATC_SAMPLE_MAX_M.
 * THE DRAW.  mean and std are [H][B*N*3] float32 (device).  For candidate m, segment h, aircraft i = e*N + k (its index in this batch)
 * and component c in {0, 1, 2} (v, h, phi), with mix64 the 64-bit mixer of the reset draws (z += 0x9E3779B97F4A7C15; z = (z ^ z >> 30) *
 * 0xBF58476D1CE4E5B9; z = (z ^ z >> 27) * 0x94D049BB133111EB; z ^ z >> 31, all modulo 2^64):
 *
 *     key = mix64( mix64(seed ^ ((u64)iteration << 32 | (u64)m)) ^ ((u64)h << 32 | (u64)i) )
 *     w   = mix64(key ^ (u64)(c + 1))
 *     S   = (w & 0xffff) + ((w >> 16) & 0xffff) + ((w >> 32) & 0xffff) + (w >> 48)            an exact integer 0 .. 262140
 *     z   = (float)((int)S - 131070) * 0x1.bb67aep-16f                                        ONE fp32 multiply
 *     a   = fminf(fmaxf(mean[h][i][c] + std[h][i][c] * z, -1.0f), 1.0f)                       two fp32 roundings, never fused
 *
 * z is a centred sum of four 16-bit uniforms (Irwin-Hall) scaled by the fp32 nearest to 1 / sqrt((65536^2 - 1) / 3): mean 0, variance
 * 1, kurtosis 2.7, support +-3.46.  With ATC_DRAW_MEAN_FIRST in dr->flags candidate 0 is the mean itself, a = fminf(fmaxf(mean, -1), 1),
 * and no key is evaluated for it.  A NaN in mean or std gives a = -1 (fmaxf returns its other operand).  The draw of (m, h, i) does
 * not depend on M, H, B or on the other candidates; another `iteration` or `seed` gives a fresh set.  Only the continuous action space
 * is drawn: both calls refuse ATC_M_DISCRETE in p->mode (atc_plan_draw takes p for that alone).
 *
 * atc_plan_draw materialises drawn plans: rows r < R of actions [R][H][B*N*3].  index == NULL: R = M and row r is candidate r.
 * Otherwise R = E and row r of env e is candidate index[r*B + e] (device pointer; indices may repeat); an env whose index is outside
 * 0 .. M-1 keeps what the row holds (atc_state_select's rule).  ATC_ERR_ARG, in this order: H outside 1 .. ATC_PLAN_MAX_H; M outside
 * 1 .. ATC_SAMPLE_MAX_M; E < 1 when index is given; a NULL pointer (s, mean, std, dr, actions, p); ATC_M_DISCRETE; B or N out of range.
 * Counted by atc_plan_draw_launch_counts only (one slot).
 *
 * atc_lookahead_plan_sampled is atc_lookahead_plan on the plans atc_plan_draw(index = NULL) would write — every word of every output
 * equal, bit for bit; no action tensor exists.  The state is untouched and the WIDE rule is atc_lookahead_plan's; draws lie in
 * [-1, 1], so no drawn action makes a heading WIDE.  ATC_ERR_ARG, in this order, the first three before any pointer is looked at: K
 * outside 1 .. ATC_SKIP_MAX; H outside 1 .. ATC_PLAN_MAX_H; M outside 1 .. ATC_SAMPLE_MAX_M; dr, mean or std NULL; out, out->reward or
 * out->done NULL; the argument errors of atc_step; ATC_M_ACTIONS_HELD or ATC_M_DISCRETE in p->mode.
 * Counted by atc_plan_sampled_launch_counts only (slot = log2(W); the rules of atc_skip_launch_counts): every other launch record stays
 * still.  atc_lookahead_set_mapping governs this call's candidates per workgroup as well; results do not depend on it. */
#define ATC_SAMPLE_MAX_M 1024
#define ATC_DRAW_MEAN_FIRST 1u
typedef struct atc_plan_draw {
    uint64_t seed;
    uint32_t iteration;
    uint32_t flags;      /* ATC_DRAW_MEAN_FIRST or 0 */
} atc_plan_draw_t;
int atc_plan_draw(const atc_scenario_t* s, int B, int N, int H, int M, const float* mean, const float* std /* [H][B*N*3] each */,
                  const atc_plan_draw_t* dr, const int32_t* index /* nullable [E][B], device */, int E,
                  float* actions /* [R][H][B*N*3] */, const atc_params_t* p, void* stream);
int atc_lookahead_plan_sampled(const atc_scenario_t* s, int B, int N, int K, int H, int M, const atc_state_t* st,
                               const float* mean, const float* std, const atc_plan_draw_t* dr,
                               const atc_plan_out_t* out, const atc_params_t* p, void* stream);
enum { ATC_PLAN_SAMPLED_LAUNCH_SLOTS = 7 };
int atc_plan_sampled_launch_counts(uint64_t* out, int n);
enum { ATC_PLAN_DRAW_LAUNCH_SLOTS = 1 };
int atc_plan_draw_launch_counts(uint64_t* out, int n);

/* atc_plan_refit: the distribution update of a sampling planner on the drawn plans, none materialised — the weighted mean and standard
 * deviation over the M candidates of one (seed, iteration), each regenerated in registers.  weight is [M][B] float32 (device): 0/1 for
 * the elites of CEM, softmax(score / lambda) for MPPI, anything else for a reward-weighted refit.  Candidate m of env e PARTICIPATES iff
 * 0 < weight[m*B + e] <= FLT_MAX: a NaN, zero, negative or infinite weight leaves it out (give weight 0 to a candidate that was not
 * evaluated, n_steps == 0).  For every segment h, aircraft i = e*N + k and component c, with a_m exactly the value atc_plan_draw writes
 * for (m, h, i, c) — same key, same ATC_DRAW_MEAN_FIRST rule, same NaN behaviour:
 *
 *     ctr = fminf(fmaxf(mean[h][i][c], -1), 1)
 *     W = 0; s1 = 0; s2 = 0
 *     for m = 0 .. M-1 ascending, participating candidates only:
 *         w = weight[m][e];  d = a_m - ctr;  t = w * d
 *         s1 = s1 + t;  s2 = s2 + t * d;  W = W + w
 *     q = s1 / W
 *     new_mean[h][i][c] = ctr + q
 *     new_std [h][i][c] = sqrtf(fmaxf(s2 / W - q * q, 0))
 *
 * Every operation is fp32 and rounded once, nothing is fused, the division and the square root are correctly rounded, and the loop is
 * sequential in m: a loop over M in any IEEE fp32 arithmetic reproduces every word (tests/plan_refit_ref.py does, in numpy).  The moments
 * are taken about ctr because their terms then scale as std * z: E[a^2] - E[a]^2 would lose a standard deviation below about 1e-3.
 * An env with no participating candidate is NOT WRITTEN: its new_mean / new_std rows keep what they hold (atc_state_select's rule).  If an
 * env's participating weights sum beyond FLT_MAX its rows are unspecified; nothing faults and no other env is affected.
 * ALIASING: new_mean == mean and new_std == std are allowed as exactly equal pointers (the in-place update: a lane reads its own words
 * before it writes them).  Any other overlap among the byte ranges of mean, std, new_mean, new_std (H*B*N*12 bytes each) and weight
 * (M*B*4 bytes) is ATC_ERR_ARG.
 * ATC_ERR_ARG, in this order, the first two before any pointer is looked at: H outside 1 .. ATC_PLAN_MAX_H; M outside 1 ..
 * ATC_SAMPLE_MAX_M; a NULL pointer (s, mean, std, dr, weight, new_mean, new_std, p); ATC_M_DISCRETE in p->mode; B or N out of range; the
 * overlap rule.  Counted by atc_plan_refit_launch_counts only (one slot); a refused call moves no launch record. */
int atc_plan_refit(const atc_scenario_t* s, int B, int N, int H, int M,
                   const float* mean, const float* std /* [H][B*N*3] each */, const atc_plan_draw_t* dr,
                   const float* weight /* [M][B], device */,
                   float* new_mean, float* new_std /* [H][B*N*3] each */,
                   const atc_params_t* p, void* stream);
enum { ATC_PLAN_REFIT_LAUNCH_SLOTS = 1 };
int atc_plan_refit_launch_counts(uint64_t* out, int n);

/* atc_plan_score: what lies between the scoring launch and the refit launch of a sampling planner's iteration, in one launch — the
 * segment rewards of the M candidates turned into a discounted score per candidate, a strict total order per env, the weights
 * atc_plan_refit reads (elite 0/1, or softmax) and the best R candidate numbers (what atc_plan_draw's `index` takes).  `s` names the
 * device, as in atc_plan_draw; the call reads nothing else of it.  All array pointers are device pointers.
 * SCORE.  g_0 = 1.0f; g_h = g_{h-1} * gamma, each one fp32 multiply.  score[m][e] = seg[m][0][e] is assigned, not 0 + ...; then for
 * h = 1 .. H-1 ascending: score = score + seg[m][h][e] * g_h.  The product and the sum are each rounded once and never fused (the file
 * is built with -ffp-contract=off).  A score that is a NaN is stored as the quiet NaN 0x7FC00000 (IEEE 754 fixes neither the sign nor
 * the payload of a computed NaN), so that every score word is defined.
 * VALID.  Candidate m of env e is VALID iff both hold: n_steps == NULL or n_steps[m*B + e] != 0; fabsf(score) <= FLT_MAX, so the score
 * is not NaN and not +-Inf.  An invalid candidate gets weight = 0 and never appears in top.  Its score word is still the computed value.
 * ORDER.  Valid candidates of an env are ordered by score descending.  Equal scores go to the LOWER candidate number.  +0 and -0
 * compare equal.  This is a strict total order.  Every result below is a function of it.
 * ELITE.  The first min(elites, number of valid candidates) candidates in the order get weight = 1.0f.  All others get 0.0f.
 * SOFTMAX.  With smax the score of the first candidate in the order:
 *
 *     x = (score - smax) / temperature          one fp32 subtraction and one correctly rounded fp32 division
 *     weight = expf(x)
 *
 * The best candidate therefore gets exactly 1.0f, since expf(0) == 1.  expf is the device library's.  It is the only inexact step in
 * the contract (tests/plan_score_ref.py restates everything else in numpy, bit for bit, and x exactly).
 * TOP.  Row r < R of env e is the candidate number at position r of the order.  The entry is -1 where the env has fewer than r+1 valid
 * candidates.  -1 is out of range for atc_plan_draw's index, so that row is kept.  R is independent of elites.  top[0] is the winner in
 * both modes.
 * ENV WITH NO VALID CANDIDATE.  All M weights are 0, which atc_plan_refit reads as "not written".  Every top entry is -1.
 * score is required: it is a result and the call's workspace.  weight is required.  Results do not depend on how the launch maps envs
 * to lanes.
 * ALIASING.  Any overlap among the byte ranges of seg_reward (M*H*B*4 bytes), n_steps (M*B*2), score, weight (M*B*4 each) and top
 * (R*B*4) is ATC_ERR_ARG (pointer values only, as atc_plan_refit compares them; ranges that only touch are accepted).
 * ATC_ERR_ARG, in this order, the first three before any pointer is looked at, atc_last_error() naming the argument: H outside 1 ..
 * ATC_PLAN_MAX_H; M outside 1 .. ATC_SAMPLE_MAX_M; R outside 0 .. ATC_SCORE_MAX_TOP, or R > 0 with top == NULL; a NULL pointer among s,
 * seg_reward, sc, score, weight; sc->mode unknown; in ELITE mode, elites outside 1 .. M; gamma not finite; in SOFTMAX mode, temperature
 * not > 0 and finite; B < 1; the overlap rule.
 * Counted by atc_plan_score_launch_counts only (one slot; the rules of atc_plan_refit_launch_counts); a refused call moves no launch
 * record. */
#define ATC_SCORE_MAX_TOP 64
enum { ATC_SCORE_ELITE = 0, ATC_SCORE_SOFTMAX = 1 };
typedef struct atc_plan_score {
    uint32_t mode;         /* ATC_SCORE_ELITE | ATC_SCORE_SOFTMAX */
    int32_t  elites;       /* ELITE: 1 .. M */
    float    gamma;        /* discount per SEGMENT, finite */
    float    temperature;  /* SOFTMAX: > 0 and finite */
} atc_plan_score_t;
int atc_plan_score(const atc_scenario_t* s, int B, int H, int M,
                   const float* seg_reward /* [M][H][B] */, const uint16_t* n_steps /* nullable [M][B] */,
                   const atc_plan_score_t* sc,
                   float* score /* [M][B], required: result and workspace */,
                   float* weight /* [M][B], required */,
                   int32_t* top /* nullable [R][B] */, int R, void* stream);
enum { ATC_PLAN_SCORE_LAUNCH_SLOTS = 1 };
int atc_plan_score_launch_counts(uint64_t* out, int n);

/* BRANCH (extension): atc_lookahead that KEEPS the outcomes — M candidate action blocks per env are flown for K steps in ONE launch and
 * each outcome becomes an env of a second batch `dst` of M*B envs, which a caller can score, expand again (beam search, MCTS expansion,
 * restore) or commit with atc_state_select instead of flying the winner a second time.  1 <= K <= ATC_SKIP_MAX, 1 <= M <=
 * ATC_LOOKAHEAD_MAX_M.  Candidate m of env e owns child env c = m*B + e of dst.  Defined per (m, e) as
 *
 *     atc_step_skip(s, B, N, K, <a bit-exact private copy of src env e>, actions[m], ..., p, stream)
 *
 * i.e. the copy steps with actions[m] until a step reports done or n == K.
 * DST STATE: the rows of child c in ac, alt, last_act, env and stats are bit for bit what that call leaves behind, the per-episode
 * record update of an auto-reset inside the call included.  A phi_wide row of dst is written only for an aircraft whose phi_fix or
 * last_act[.][1] is saturated; every other phi_wide row of dst is unspecified (as atc_state_t allows: its contents are unspecified
 * while the 32-bit fields are in range).
 * OUT: atc_lookahead_out_t with atc_lookahead's meaning, word for word: reward and done are required, every other pointer may be
 * NULL; [M][B...] is the child batch's own [M*B...] layout, so the child env's bound output tensors can be passed; a launch that asks
 * for neither ac_reward nor min_sep runs a form with those two compiled out (obs and flags, what a child env always binds, are stored
 * by both forms where requested, as atc_step_skip's fast form stores them).  There is no term_obs.
 * RESET DRAWS inside the call use the SOURCE env index e and the copy's episode number, like atc_lookahead — which is what makes the
 * call equal to atc_step_skip on a copy of src.  Afterwards dst is an ordinary batch: later resets of child c are keyed by c.
 * ATC_M_ACTIONS_HELD afterwards: the previous step of child c is this call's step with actions[m] — an atc_step of dst with those
 * actions may set the bit (a child that ended and was reset inside the call has timesteps == 0 and is handled in full); the previous
 * step of a child that was NOT EVALUATED (below) is src env e's previous step.
 * SRC is read only: all six arrays are byte-identical afterwards.
 * LIMIT — WIDE headings: atc_lookahead's rule.  An env-candidate that is WIDE at the start (phi_fix or last_act[.][1] of any aircraft
 * saturated) or becomes WIDE in an executed step is NOT EVALUATED: n_steps = 0, done = 0, every requested output word of (m, e) is 0,
 * and child c is a byte copy of src env e's rows — the phi_wide rows of its saturated aircraft included.
 * ATC_ERR_ARG, in this order, the first two before any pointer is looked at: K outside 1 .. ATC_SKIP_MAX; M outside 1 ..
 * ATC_LOOKAHEAD_MAX_M; out, out->reward or out->done NULL; dst NULL or any of its six pointers NULL; any dst array's byte range (sized
 * for M*B envs) overlaps any src array's range (sized for B envs); M*B not a batch size atc_step accepts; the argument errors of
 * atc_step; ATC_M_ACTIONS_HELD in p->mode.
 * Counted by atc_branch_launch_counts only (slot = log2(W); the rules of atc_skip_launch_counts): every other launch record stays
 * still.  atc_lookahead_set_mapping governs this call's candidates per workgroup as well; results do not depend on it. */
int atc_branch(const atc_scenario_t* s, int B, int N, int K, int M, const atc_state_t* src, const float* actions /* [M][B*N*3] */,
               const atc_state_t* dst /* M*B envs */, const atc_lookahead_out_t* out, const atc_params_t* p, void* stream);
enum { ATC_BRANCH_LAUNCH_SLOTS = 7 };
int atc_branch_launch_counts(uint64_t* out, int n);

/* SELECT (extension): gather env states between batches by index — the other half of atc_branch (commit a winner, keep a beam,
 * restore a snapshot).  For every e < B_dst with mask[e] != 0 (mask NULL: every e) and 0 <= index[e] < B_src, dst env e takes src env
 * index[e]'s rows of ac, alt, last_act, env and stats, and the phi_wide row of each aircraft with a saturated field (phi_fix or
 * last_act[.][1]).  Every other dst byte is untouched: envs masked out and envs with a negative or too-large index keep what they
 * hold.  Indices may repeat.  No arithmetic, no parameters, no random numbers; index and mask are device pointers.
 * ATC_M_ACTIONS_HELD afterwards: the previous step of a written dst env is the previous step of the src env it was gathered from (its
 * last_act row came along); an env that was not written keeps its own.
 * src and dst may not overlap (atc_branch's range check).  ATC_ERR_ARG: N outside 1 .. 64 or B_dst / B_src < 1 (checked first); index
 * NULL, a NULL state pointer, overlapping arrays.  Counted by atc_select_launch_counts only (one slot). */
int atc_state_select(const atc_scenario_t* s, int N, int B_dst, const atc_state_t* dst, int B_src, const atc_state_t* src,
                     const int32_t* index /* [B_dst], device */, const uint8_t* mask /* nullable [B_dst] */, void* stream);
enum { ATC_SELECT_LAUNCH_SLOTS = 1 };
int atc_select_launch_counts(uint64_t* out, int n);

/* POLICY ROLLOUT (extension): the on-policy collection loop of the reference's trainer — PPO2 with MlpPolicy, two tanh layers of 64 and
 * a diagonal Gaussian, n_steps transitions per update (learning/atc-gym-stable-baselines.py:112-122) — in ONE launch: observation ->
 * MLP -> Gaussian sample -> clamp -> step, T times, the state in registers throughout like atc_rollout_hold.  The action of step t + 1
 * depends on the observation of step t, so a caller of atc_step pays a launch boundary (and half a dozen framework launches) inside
 * every step.  The policy is 10 -> 64 -> 64 -> 3: ATC_POLICY_WORDS floats in one device array, each weight matrix row-major
 * [out][in], i.e. torch.nn.Linear.weight as it lies in memory.  A value head is not part of it: values come from one batched forward
 * over the stored observations.
 * DECISIONS.  Decision b, for b = 0 .. T / hold - 1, is taken for every aircraft slot i = e*N + k from the ten words x that the step
 * before it stored for that slot: obs0 for b = 0, out->obs of step b*hold - 1 otherwise — exactly what a caller of atc_step would feed
 * its policy (normalised or not per ATC_M_NORMALIZE, the raw reset observation right after an auto-reset, zeros for an aircraft that
 * is not under control).  With mix64 the mixer of the reset draws (see atc_plan_draw):
 *
 *     h1 = tanh(W1 x + b1);  h2 = tanh(W2 h1 + b2);  mu = W3 h2 + b3;  sigma_c = expf(log_std_c)
 *     key = mix64( mix64(seed ^ (u64)(decision0 + b)) ^ (u64)i )         decision0 + b wraps modulo 2^32
 *     w_c = mix64(key ^ (u64)(c + 1))                                    c = 0, 1, 2 (v, h, phi)
 *     u1  = ((w_c >> 40) + 1) * 2^-24   in (0, 1];    u2 = ((w_c >> 16) & 0xffffff) * 2^-24   in [0, 1)
 *     z_c = sqrtf(-2 logf(u1)) * cosf(2 pi u2)                           Box-Muller: a true Gaussian, |z| <= 5.77; 2 pi u2 is ONE fp32
 *                                                                        product with the fp32 nearest to 2 pi
 *     u_c = mu_c + sigma_c * z_c                                         ATC_POLICY_DETERMINISTIC: u_c = mu_c, no key is evaluated, logp = 0
 *     a_c = fminf(fmaxf(u_c, -1), 1)                                     a NaN (a diverged network) gives -1: no NaN reaches the env
 *     logp = sum_c (-0.5 z_c^2 - log_std_c) - 1.5 log(2 pi)              the log-density of u under N(mu, sigma)
 *
 * action[b] = u, the UNCLAMPED sample (what logp is about), and logp[b] as above; steps b*hold .. b*hold + hold - 1 are flown with a.
 * Successive launches pass decision0 += T / hold for fresh noise, and the last observation of one launch as the obs0 of the next: two
 * launches of T / 2 then reproduce one launch of T bit for bit.
 * DYNAMICS.  Everything else — the per-step outputs, the state afterwards, stepping through auto-resets inside a held block, the
 * last-action record, WIDE headings — is atc_rollout_hold(T, hold) on the tensor of the clamped actions a, bit for bit.
 * EXACT AND INEXACT.  The integers, the key, u1 and u2 are exact.  The dot products may be summed in any order and by any unit; tanh,
 * expf, logf and cosf are the device library's, not the fast intrinsics: mu, z, u and logp are values (tests/policy_ref.py restates them
 * in float64 and states the bars), a is exactly the clamp of the stored u.
 * ATC_ERR_ARG, in this order, the first before any pointer is looked at, atc_last_error() naming the argument: T < 1, hold < 1 or T not
 * a multiple of hold; a NULL among pol, pol->w, obs0, out, out's four step outputs, out->action; n_hidden != ATC_POLICY_HIDDEN or
 * unknown flag bits; the argument errors of atc_rollout_hold; ATC_M_DISCRETE (a Gaussian policy draws the continuous space only) or
 * ATC_M_ACTIONS_HELD in p->mode; obs0 (B*N*40 bytes) overlapping out->obs (T*B*N*40 bytes).
 * Counted by atc_rollout_policy_launch_counts only (slot = log2(W); the rules of atc_skip_launch_counts): every other launch record
 * stays still, and a refused call moves none. */
#define ATC_POLICY_IN 10            /* = ATC_OBS_DIM: the policy sees one aircraft's own observation row */
#define ATC_POLICY_HIDDEN 64
#define ATC_POLICY_WORDS 5062
#define ATC_POLICY_DETERMINISTIC 1u
typedef struct atc_policy {
    const float* w;      /* device, ATC_POLICY_WORDS floats: W1[64][10], b1[64], W2[64][64], b2[64], W3[3][64], b3[3], log_std[3] */
    int32_t n_hidden;    /* must be ATC_POLICY_HIDDEN (refused otherwise; the field is there so a later width needs no new struct) */
    uint32_t flags;      /* ATC_POLICY_DETERMINISTIC or 0 */
    uint64_t seed;
    uint32_t decision0;  /* number of the launch's first decision */
    uint32_t reserved;
} atc_policy_t;
typedef struct atc_policy_out {
    float* obs;          /* [T][B*N*10]     required: atc_rollout's per-step outputs */
    float* reward;       /* [T][B]          required */
    uint8_t* done;       /* [T][B]          required */
    uint16_t* flags;     /* [T][B*N]        required */
    float* action;       /* [T/hold][B*N*3] required: the UNCLAMPED sample u */
    float* logp;         /* [T/hold][B*N]   nullable */
} atc_policy_out_t;
int atc_rollout_policy(const atc_scenario_t* s, int B, int N, int T, int hold, const atc_state_t* st,
                       const float* obs0 /* [B*N*10] */, const atc_policy_t* pol, const atc_policy_out_t* out,
                       const atc_params_t* p, void* stream);
enum { ATC_ROLLOUT_POLICY_LAUNCH_SLOTS = 7 };
int atc_rollout_policy_launch_counts(uint64_t* out, int n);

/* POLICY ROLLOUT WITH TRAFFIC (extension): atc_rollout_policy whose policy also sees the traffic observation — the multi-aircraft
 * envs punish lost separation that none of the ten own words shows.  The traffic query of atc_observe_traffic(K) is evaluated INSIDE the
 * launch, at every decision, on the state the loop holds; it feeds a wider first layer, IN -> 64 -> 64 -> 3 with IN = 10 + 7 K
 * (ATC_POLICY_TRAFFIC_IN), and the records each decision saw are stored so that a trainer can recompute logp in its update.
 * K = traffic_k is 1, 2 or 4 (the compiled list lengths).  The weights are ONE device array of ATC_POLICY_TRAFFIC_WORDS(K) = 4422 + 64 IN
 * floats (5510, 5958, 6854), laid out exactly like ATC_POLICY_WORDS with W1[64][IN] row-major.
 * INPUT ROW.  Aircraft slot i at decision b sees  x = [ own ten words | record 0 words 0..6 | ... | record K-1 words 0..6 ]:
 *   - the own words are exactly atc_rollout_policy's: obs0 for b = 0, the observation step b*hold - 1 stored otherwise;
 *   - the records are exactly what atc_observe_traffic(K) returns for the state the env is in when the decision is taken: the state at
 *     launch for b = 0, otherwise the state step b*hold - 1 left — the fresh spawn after an auto-reset (the convention of
 *     AtcVecEnv's info["traffic"]); normalised or not per ATC_M_NORMALIZE, like the own words;
 *   - word 7 of a record (the slot) is stored but is not an input.
 * THE TRAFFIC HALF IS EXACT.  out->traffic[b] equals atc_observe_traffic(K) on that state bit for bit: selection by
 * (bits(d^2) << 32 | slot), ABSENT ranks, WIDE headings wrapped — everything stated under TRAFFIC OBSERVATION.
 * EVERYTHING ELSE is atc_rollout_policy's contract, unchanged: the same key, Box-Muller and logp; action is the unclamped sample; the
 * dynamics are atc_rollout_hold on the clamped actions bit for bit; two launches of T / 2 with decision0 += T / (2 hold) and obs0
 * chained reproduce one launch of T bit for bit, `traffic` included.
 * FLOAT64 LAYER 1.  A wavefront that holds an input above 4 in magnitude, or a NaN, sums layer 1 in float64; the rule is applied over
 * the whole widened row, so unnormalised records (nm, ft, kt) take it.
 * ATC_ERR_ARG: the refusals of atc_rollout_policy in its order; traffic_k outside {1, 2, 4} is refused behind n_hidden, naming the
 * field; the overlap rule also refuses out->traffic (T/hold * B*N*K*32 bytes) sharing memory with obs0, out->obs or one of the six
 * state arrays.
 * Counted by atc_rollout_policy_traffic_launch_counts only: slot = 3 log2(W) + log2(K). */
#define ATC_POLICY_TRAFFIC_IN(K) (10 + 7 * (K))                  /* own row + words 0..6 of K records */
#define ATC_POLICY_TRAFFIC_WORDS(K) (4422 + 64 * ATC_POLICY_TRAFFIC_IN(K))
typedef struct atc_policy_traffic {
    const float* w;      /* device, ATC_POLICY_TRAFFIC_WORDS(traffic_k) floats: W1[64][IN], b1[64], W2[64][64], b2[64], W3[3][64], b3[3], log_std[3] */
    int32_t n_hidden;    /* must be ATC_POLICY_HIDDEN */
    uint32_t flags;      /* ATC_POLICY_DETERMINISTIC or 0 */
    uint64_t seed;
    uint32_t decision0;  /* number of the launch's first decision */
    uint32_t reserved;
    int32_t traffic_k;   /* K: 1, 2 or 4 records per aircraft (atc_rollout_policy_ends: also 0, the ten-word policy) */
} atc_policy_traffic_t;
typedef struct atc_policy_traffic_out {
    float* obs;          /* [T][B*N*10]     required: atc_rollout's per-step outputs */
    float* reward;       /* [T][B]          required */
    uint8_t* done;       /* [T][B]          required */
    uint16_t* flags;     /* [T][B*N]        required */
    float* action;       /* [T/hold][B*N*3] required: the UNCLAMPED sample u */
    float* logp;         /* [T/hold][B*N]   nullable */
    float* traffic;      /* [T/hold][B*N*K*8] nullable: the records decision b saw, in atc_observe_traffic's layout */
} atc_policy_traffic_out_t;
int atc_rollout_policy_traffic(const atc_scenario_t* s, int B, int N, int T, int hold, const atc_state_t* st,
                               const float* obs0 /* [B*N*10] */, const atc_policy_traffic_t* pol, const atc_policy_traffic_out_t* out,
                               const atc_params_t* p, void* stream);
enum { ATC_ROLLOUT_POLICY_TRAFFIC_LAUNCH_SLOTS = 21 };
int atc_rollout_policy_traffic_launch_counts(uint64_t* out, int n);

/* POLICY ROLLOUT WITH EPISODE ENDS (extension): atc_rollout_policy and atc_rollout_policy_traffic behind one entry point, with the three
 * per-decision outputs a trainer cannot rebuild from the [T] arrays: the env is reset INSIDE the step that ends its episode, so the
 * observation of the state the episode ended in, and which aircraft a decision controlled, never leave the other two launches.
 * pol->traffic_k is 0, 1, 2 or 4.  0 is the ten-word policy of atc_rollout_policy (ATC_POLICY_TRAFFIC_WORDS(0) == ATC_POLICY_WORDS; no
 * traffic query is evaluated, and out->traffic must be NULL: refused otherwise, naming the field); 1, 2, 4 is atc_rollout_policy_traffic.
 * ENDING STEP.  With D = T / hold, decision d owns steps d*hold .. d*hold + hold - 1; its ending step t* is the first of them with
 * done != 0 for that env — atc_gae's BLOCK rule and atc_step_skip's: a transition never spans two episodes.
 *   - term_obs[d], the env's N rows: written only where block d has an ending step — the observation of the state step t* ENDED in, bit
 *     for bit what atc_rollout_hold writes to out->term_obs of step t* under ATC_M_AUTO_RESET (normalised or not like obs, zeros for an
 *     aircraft not under control); without ATC_M_AUTO_RESET it is obs of step t*.  The rows of an env whose block has no ending step are
 *     NOT written and keep what they hold; a second episode end inside the same block writes nothing.
 *   - term_flags[d][e], written for every env and decision: 0 where block d has no ending step, otherwise ATC_TERM_ENDED OR-ed with the
 *     flag words of the env's N aircraft at step t*, exactly as flags[t*] stores them (the defined flag bits end at bit 9).  A time-limit
 *     end reads as ATC_F_TIMEOUT set with ATC_F_BELOW_MVA | ATC_F_OUTSIDE | ATC_F_CONFLICT clear: the one end a trainer bootstraps
 *     (atc_gae_boot).
 *   - control[d][i] = 1 iff aircraft i's bit of its env's active mask (ATC_ENV_MASK_LO / ATC_STAT_MASK_HI) is set in the state decision d
 *     is taken in: the state at launch for d = 0, otherwise what step d*hold - 1 left — all ones after an auto-reset.  The predicate the
 *     traffic query ranks by.
 * EVERYTHING ELSE is the contract of the two calls, word for word: every other output, the key, the draw, logp, traffic, the dynamics and
 * the state afterwards are bit-identical to theirs for the same arguments, and two launches of T / 2 equal one of T bit for bit, the
 * three outputs included.
 * ATC_ERR_ARG: the refusals of atc_rollout_policy_traffic in its order (traffic_k outside {0, 1, 2, 4}; behind the flag bits, a non-NULL
 * out->traffic with traffic_k == 0); the overlap rule also refuses term_obs (T/hold * B*N*40 bytes), term_flags (T/hold * B*2) or control
 * (T/hold * B*N) sharing memory with obs0, out->obs, a state array, out->traffic or one another.
 * Counted by atc_rollout_policy_ends_launch_counts only: slot = 4 log2(W) + {0, 1, 2, 3 for K = 0, 1, 2, 4}. */
#define ATC_TERM_ENDED 0x8000u       /* term_flags: block d has an ending step */
typedef struct atc_policy_ends_out {
    float* obs;          /* [T][B*N*10]     required: atc_rollout's per-step outputs */
    float* reward;       /* [T][B]          required */
    uint8_t* done;       /* [T][B]          required */
    uint16_t* flags;     /* [T][B*N]        required */
    float* action;       /* [T/hold][B*N*3] required: the UNCLAMPED sample u */
    float* logp;         /* [T/hold][B*N]   nullable */
    float* traffic;      /* [T/hold][B*N*K*8] nullable; must be NULL with traffic_k == 0 */
    float* term_obs;     /* [T/hold][B*N*10] nullable: rows of envs whose block ended, the others are left as they are */
    uint16_t* term_flags;/* [T/hold][B]     nullable: 0, or ATC_TERM_ENDED | the OR of the env's flag words at the ending step */
    uint8_t* control;    /* [T/hold][B*N]   nullable: 1 = under control when the decision was taken */
} atc_policy_ends_out_t;
int atc_rollout_policy_ends(const atc_scenario_t* s, int B, int N, int T, int hold, const atc_state_t* st,
                            const float* obs0 /* [B*N*10] */, const atc_policy_traffic_t* pol, const atc_policy_ends_out_t* out,
                            const atc_params_t* p, void* stream);
enum { ATC_ROLLOUT_POLICY_ENDS_LAUNCH_SLOTS = 28 };
int atc_rollout_policy_ends_launch_counts(uint64_t* out, int n);

/* POLICY ROLLOUT WITH TERMINAL TRAFFIC RECORDS (extension): atc_rollout_policy_ends for a policy that sees traffic (pol->traffic_k = K in
 * {1, 2, 4}), with one more nullable per-decision output.  A critic over 10 + 7 K inputs bootstraps a time-limit end from the row
 * [term_obs | words 0..6 of the K records of that state]; the auto-reset inside the ending step overwrites the state, so the records, like
 * term_obs, can only be taken inside the launch.
 *   - term_traffic[d], the env's N x K records: written only where block d has an ending step t* (ENDING STEP above) — bit for bit what
 *     atc_observe_traffic(K) returns on the state step t* ENDED in, the state term_obs[d] describes: after that step's kinematics, with the
 *     aircraft the step handed over taken out of the active mask (they are not under control: absent as intruders, all-ABSENT as
 *     observers), ahead of the spawn.  Without ATC_M_AUTO_RESET it is atc_observe_traffic on the state step t* left.  The rows of an env
 *     whose block has no ending step are NOT written and keep what they hold; a second episode end inside the same block writes nothing.
 *   - WIDE headings: an aircraft whose terminal heading is WIDE (ABI 19) is rotated by its exact counts, as atc_observe_traffic reads them
 *     from the side record — the reset writes no side record, and the launch reads the row before any later step can.
 * EVERYTHING ELSE is atc_rollout_policy_ends' contract word for word: every other output and the state afterwards are bit-identical to that
 * call's for the same arguments, with term_traffic given or NULL, and two launches of T / 2 equal one of T bit for bit, term_traffic
 * included.  All stores are plain vector stores.
 * ATC_ERR_ARG, in this order: T and hold; the pointers (pol, pol->w, obs0, out; obs / reward / done / flags; action); n_hidden; traffic_k
 * outside {1, 2, 4} (0 is refused: the ten-word policy has no records — atc_rollout_policy_ends); the flag bits; the argument errors of
 * atc_rollout_hold that need no sector (s, st, p, the batch shape, a null state field, the batch size); ATC_M_DISCRETE; ATC_M_ACTIONS_HELD;
 * the overlap rule of atc_rollout_policy_ends; then term_traffic (T/hold * B*N*K*32 bytes) sharing memory with pol->w, obs0, any other
 * output of the call or one of the six state arrays (ranges that only touch do not overlap); LAST the time increment (dt), the one refusal
 * that reads the sector — everything in front of it looks at s for NULL only.
 * Counted by atc_rollout_policy_term_launch_counts only: slot = 3 log2(W) + log2(K); a refused call moves no record. */
typedef struct atc_policy_term_out {
    float* obs;          /* [T][B*N*10]     required: atc_rollout's per-step outputs */
    float* reward;       /* [T][B]          required */
    uint8_t* done;       /* [T][B]          required */
    uint16_t* flags;     /* [T][B*N]        required */
    float* action;       /* [T/hold][B*N*3] required: the UNCLAMPED sample u */
    float* logp;         /* [T/hold][B*N]   nullable */
    float* traffic;      /* [T/hold][B*N*K*8] nullable: the records decision b saw */
    float* term_obs;     /* [T/hold][B*N*10] nullable: rows of envs whose block ended, the others are left as they are */
    uint16_t* term_flags;/* [T/hold][B]     nullable: 0, or ATC_TERM_ENDED | the OR of the env's flag words at the ending step */
    uint8_t* control;    /* [T/hold][B*N]   nullable: 1 = under control when the decision was taken */
    float* term_traffic; /* [T/hold][B*N*K*8] nullable: the records of the state term_obs describes, rows of envs whose block ended */
} atc_policy_term_out_t;
int atc_rollout_policy_term(const atc_scenario_t* s, int B, int N, int T, int hold, const atc_state_t* st,
                            const float* obs0 /* [B*N*10] */, const atc_policy_traffic_t* pol, const atc_policy_term_out_t* out,
                            const atc_params_t* p, void* stream);
enum { ATC_ROLLOUT_POLICY_TERM_LAUNCH_SLOTS = 21 };
int atc_rollout_policy_term_launch_counts(uint64_t* out, int n);

/* POLICY EVALUATION (extension): how good is this policy?  The reference's trainer logs winning_ratio, the mean episode length and
 * Monitor's r / l after every update (learning/atc-gym-stable-baselines.py).  atc_policy_eval flies a packed policy for T steps exactly as
 * atc_rollout_policy_ends does — the decisions, the key, the draw, the clamp, ATC_POLICY_DETERMINISTIC, the traffic query for traffic_k > 0,
 * held blocks stepping through auto-resets, and the state afterwards (the per-episode record included) are that call's, bit for bit — and
 * stores NONE of its per-step or per-decision streams.  What leaves the launch is one record of ATC_EVAL_WORDS 32-bit words per env
 * (float words by bit pattern), and optionally the last step's observation.
 * THE RECORD ACCUMULATES.  The launch reads out->record at its start — or, under ATC_EVAL_CLEAR, takes the initial values below without
 * reading — and writes it once at its end.  An ENDING STEP is any step of the launch with done set for the env; every one counts, also a
 * second one inside a held block (evaluation counts episodes, not transitions).  `seen` is the OR of the env's valid aircraft's flag words
 * at that step, as atc_rollout's flags[t] stores them; r and the length are the words that step writes to ATC_STAT_EP_RETURN and
 * ATC_STAT_EP_LENGTH, the win bit the one it shifts into ATC_STAT_WIN_BITS.  They are the whole episode's: an episode that began before
 * the launch (ATC_ENV_TIMESTEPS / ATC_ENV_TOTAL_REWARD carried in the state) is counted in full, one still running at the end of the
 * launch is not counted and stays in the state.  Hence two launches of T / 2 on the same record — the second with decision0 + T / (2 hold),
 * obs0 = the first's obs_last and no ATC_EVAL_CLEAR — equal one launch of T bit for bit: record, obs_last and state.
 * Every float operation is fp32, rounded once, never fused: sum = sum + r; sq = sq + (r * r); fminf / fmaxf.
 * ATC_ERR_ARG: the refusals of atc_rollout_policy_ends in its order, with out->record in the place of its required outputs; behind the
 * ATC_M_DISCRETE / ATC_M_ACTIONS_HELD refusals, ATC_M_AUTO_RESET missing from p->mode (without the reset inside the step the per-episode
 * words are never formed) and unknown bits in out->flags; then record (B * 64 bytes) or obs_last (B*N*40 bytes) sharing memory with obs0,
 * each other or one of the six state arrays.
 * Counted by atc_policy_eval_launch_counts only: slot = 4 log2(W) + {0, 1, 2, 3 for K = 0, 1, 2, 4}; a refused call moves no record. */
enum {
    ATC_EVAL_EPISODES = 0,        /* i32  + 1 at every ending step */
    ATC_EVAL_WINS = 1,            /* i32  + the bit that step shifts into ATC_STAT_WIN_BITS */
    ATC_EVAL_END_BELOW_MVA = 2,   /* i32  + 1 if `seen` has ATC_F_BELOW_MVA (an end can count in several of the four) */
    ATC_EVAL_END_OUTSIDE = 3,     /* i32  ... ATC_F_OUTSIDE */
    ATC_EVAL_END_CONFLICT = 4,    /* i32  ... ATC_F_CONFLICT */
    ATC_EVAL_END_TIMEOUT = 5,     /* i32  ... ATC_F_TIMEOUT */
    ATC_EVAL_STEPS = 6,           /* i32  + the ended episode's length */
    ATC_EVAL_RETURN_SUM = 7,      /* f32  sum = sum + r */
    ATC_EVAL_RETURN_SQ = 8,       /* f32  sq = sq + (r * r) */
    ATC_EVAL_RETURN_MIN = 9,      /* f32  fminf(min, r); initially +inf */
    ATC_EVAL_RETURN_MAX = 10,     /* f32  fmaxf(max, r); initially -inf */
    ATC_EVAL_FLAGS_OR = 11,       /* u32  the OR of the env's valid aircraft's flag words at EVERY step of the launch */
    ATC_EVAL_LAUNCH_STEPS = 12,   /* i32  + T, once per launch */
    ATC_EVAL_WORDS = 16           /* words 13 .. 15 are reserved: written as read, 0 under ATC_EVAL_CLEAR */
};
#define ATC_EVAL_CLEAR 1u
typedef struct atc_policy_eval_out {
    int32_t* record;     /* [B][ATC_EVAL_WORDS] required */
    float* obs_last;     /* [B*N*10]            nullable: the observation the last step stored, the next launch's obs0 */
    uint32_t flags;      /* ATC_EVAL_CLEAR or 0 */
} atc_policy_eval_out_t;
int atc_policy_eval(const atc_scenario_t* s, int B, int N, int T, int hold, const atc_state_t* st,
                    const float* obs0 /* [B*N*10] */, const atc_policy_traffic_t* pol, const atc_policy_eval_out_t* out,
                    const atc_params_t* p, void* stream);
enum { ATC_POLICY_EVAL_LAUNCH_SLOTS = 28 };
int atc_policy_eval_launch_counts(uint64_t* out, int n);

/* GAE (extension): what lies between the collection launch and the update of an on-policy trainer, in one launch — the per-step
 * rewards and dones of a rollout (atc_rollout_policy's reward [T][B] and done [T][B]) and the values of one batched forward turned into
 * generalised advantage estimates and returns, one transition per DECISION.  A pure function of its arrays: `s` names the device only,
 * as in atc_plan_score; no state, no parameters and no random numbers are read.  All array pointers are device pointers.
 * SIZES.  D >= 1 decisions of `hold` steps each (1 .. ATC_SKIP_MAX), T = D * hold steps.  NV = 1 .. 64 value columns per env (a
 * per-aircraft critic has N, a centralised one 1); C = B * NV columns, column i = e * NV + k.  values is [D + 1][C]: row d is the value
 * of the state decision d was taken in, row D that of the state after the last step.
 * Every operation below is fp32, rounded once and never fused (the file is built with -ffp-contract=off).
 * BLOCK.  Decision d owns steps t0 = d * hold .. t0 + hold - 1; r_t is reward[t][e], or reward[t][i] under ATC_GAE_REWARD_PER_COLUMN.
 *
 *     g = 1.0f;  R = r_{t0}  (assigned, not 0 + ...);  n = 1;  term = done[t0][e] != 0
 *     for j = 1 .. hold - 1 while !term:
 *         default:               g = g * gamma;  R = R + (r_{t0+j} * g)
 *         ATC_GAE_PER_DECISION:  R = R + r_{t0+j}
 *         n = n + 1;  term = done[t0+j][e] != 0
 *
 * Rewards and dones BEHIND THE FIRST DONE of a block are not read into anything: they belong to the next episode, flown under the old
 * decision — atc_step_skip's rule ("a transition never spans two episodes") applied to a rollout's arrays.  Any word may stand there, a
 * NaN included, without changing an output word.
 * CONSTANTS.  G = g_{hold-1} * gamma with g_j the running product above (g_0 = 1.0f, g_j = g_{j-1} * gamma), so G is exactly gamma for
 * hold == 1; under ATC_GAE_PER_DECISION G = gamma: summed rewards with the discount per decision, what a frame-skipping env in front
 * of a trainer computes.  c = G * lam, one product.
 * RECURRENCE.  d descends from D - 1.  A_next starts as adv_next[i], or +0.0f where adv_next == NULL (the operations are carried out
 * all the same).  With V = values:
 *
 *     term:   delta = R - V[d][i];                       A = delta
 *     else:   delta = (R + (G * V[d+1][i])) - V[d][i];   A = delta + (c * A_next)
 *     adv[d][i] = A;  ret[d][i] = A + V[d][i];  A_next = A
 *
 * block_reward[d] = R, block_done[d] = term, block_steps[d] = n, each stored only where its pointer is given.  A NaN is stored as the
 * quiet NaN 0x7FC00000 in adv, ret and block_reward (atc_plan_score's rule: IEEE 754 fixes neither the sign nor the payload of a
 * computed NaN).  Results do not depend on how the launch maps columns to lanes; a loop in any IEEE fp32 arithmetic reproduces every
 * word (tests/gae_ref.py does, in numpy).
 * SPLITTING.  A call on decisions D/2 .. D-1 (values + (D/2) * C, the later half of reward and done), then a call on decisions
 * 0 .. D/2 - 1 with adv_next = the first call's adv row 0, equal one call of D bit for bit.
 * TIME-LIMIT ENDS AND THE CONTROL MASK.  atc_gae treats every done as a true terminal state.  atc_gae_boot (below) bootstraps the ends
 * the caller marks as truncated from the value of the terminal observation, which atc_rollout_policy_ends stores together with the mask
 * of the aircraft each decision controlled.  NOT COVERED (the trainer's): advantage normalisation — with that mask in hand three
 * reductions over [D][B][N] — and the traffic records of a terminal state, which no launch produces.
 * ATC_ERR_ARG, in this order, the first four before any pointer is looked at, atc_last_error() naming the argument: D < 1; hold
 * outside 1 .. ATC_SKIP_MAX; NV outside 1 .. 64; B < 1; a NULL among s, reward, done, values, g, out, out->adv, out->ret; unknown flag
 * bits; gamma or lam not finite; any overlap among the byte ranges of reward (T*B*4 bytes, T*C*4 per column), done (T*B), values
 * ((D+1)*C*4), adv_next (C*4), adv, ret (D*C*4 each), block_reward (D*B*4, D*C*4 per column), block_done and block_steps (D*B each) —
 * pointer values only, ranges that only touch are accepted; B * NV beyond what one launch covers (2^31 - 1 workgroups of 64 columns).
 * Counted by atc_gae_launch_counts only (one slot; the rules of atc_plan_refit_launch_counts); a refused call moves no launch record. */
#define ATC_GAE_PER_DECISION 1u        /* block reward = plain sum, G = gamma */
#define ATC_GAE_REWARD_PER_COLUMN 2u   /* reward is [T][C]; block_reward is [D][C] */
#define ATC_GAE_MAX_NV 64
typedef struct atc_gae {
    float    gamma;   /* finite */
    float    lam;     /* finite */
    uint32_t flags;   /* ATC_GAE_PER_DECISION | ATC_GAE_REWARD_PER_COLUMN; unknown bits refused */
    uint32_t _pad;
} atc_gae_t;
typedef struct atc_gae_out {
    float*   adv;           /* [D][C] required */
    float*   ret;           /* [D][C] required */
    float*   block_reward;  /* nullable: [D][B], or [D][C] under ATC_GAE_REWARD_PER_COLUMN */
    uint8_t* block_done;    /* nullable [D][B] */
    uint8_t* block_steps;   /* nullable [D][B] */
} atc_gae_out_t;
int atc_gae(const atc_scenario_t* s, int B, int NV, int D, int hold,
            const float* reward /* [T][B], or [T][C] per column */, const uint8_t* done /* [T][B] */,
            const float* values /* [D+1][C] */, const float* adv_next /* nullable [C] */,
            const atc_gae_t* g, const atc_gae_out_t* out, void* stream);
enum { ATC_GAE_LAUNCH_SLOTS = 1 };
int atc_gae_launch_counts(uint64_t* out, int n);

/* GAE WITH BOOTSTRAPPED TRUNCATIONS (extension): atc_gae plus two inputs — boot [D][C], the value of the state block d ENDED in (the
 * critic on atc_rollout_policy_ends' term_obs[d]), and trunc [D][B], non-zero where that end is a truncation (a time limit) and not a
 * terminal state.  With g the running product at the block's last counted step (1.0f throughout under ATC_GAE_PER_DECISION):
 *
 *     term and trunc[d][e] != 0:  Gn = g * gamma;  delta = (R + (Gn * boot[d][i])) - V[d][i];  A = delta
 *     term and trunc[d][e] == 0:  as atc_gae
 *     not term:                   as atc_gae (trunc is not looked at)
 *
 * fp32, every operation rounded once, like atc_gae.  Gn is G where the block ran all `hold` steps, and gamma under ATC_GAE_PER_DECISION.
 * The episode still ends there: A_next does not enter.  A boot word is read into an output only where term and trunc both hold: anywhere
 * else it may be a NaN without changing an output word.  With boot == NULL and trunc == NULL the call equals atc_gae bit for bit; one
 * NULL without the other is ATC_ERR_ARG, refused behind the other NULL checks.  boot (D*C*4 bytes) and trunc (D*B) join atc_gae's
 * overlap rule, SPLITTING holds unchanged (boot and trunc split like reward's rows: by decision), and every other refusal is atc_gae's in
 * its order.  Counted by atc_gae_boot_launch_counts only (one slot). */
int atc_gae_boot(const atc_scenario_t* s, int B, int NV, int D, int hold,
                 const float* reward /* [T][B], or [T][C] per column */, const uint8_t* done /* [T][B] */,
                 const float* values /* [D+1][C] */, const float* adv_next /* nullable [C] */,
                 const float* boot /* nullable [D][C] */, const uint8_t* trunc /* nullable [D][B], with boot */,
                 const atc_gae_t* g, const atc_gae_out_t* out, void* stream);
enum { ATC_GAE_BOOT_LAUNCH_SLOTS = 1 };
int atc_gae_boot_launch_counts(uint64_t* out, int n);

/* PPO POLICY GRADIENT (extension): the policy half of a PPO update in one call — the clipped surrogate loss of the 10 + 7 K -> 64 -> 64 -> 3
 * policy of atc_rollout_policy_ends on stored decisions, and its gradient with respect to every word of the packed weight array, summed over
 * the rows of a minibatch.  No activation is written to global memory: the forward and the backward of a row stay in one workgroup.  A pure
 * function of its arrays, like atc_gae: `s` names the device only.  All array pointers are device pointers.
 * ROWS.  R_src source rows, R rows to evaluate.  Row i evaluates source row index[i]; an index outside [0, R_src) is skipped: it is not
 * counted and nothing of it is read.  index == NULL means R == R_src and the identity.  A row PARTICIPATES if its source row is in range and
 * mask is NULL or mask[source row] != 0 (atc_rollout_policy_ends' control, flattened).  A row that does not participate is taken out by
 * selects, never by a product with zero: any word may stand in it, a NaN included, without changing an output bit.
 * INPUT ROW.  x = obs_rows[row][0..9], then words 0..6 of each of the K = traffic_k records traffic[row][r][0..7] (word 7 is not read):
 * atc_rollout_policy_traffic's INPUT ROW.  w is the packed policy, ATC_POLICY_TRAFFIC_WORDS(K) floats.
 * PER PARTICIPATING ROW, in fp32, with u = action[row] (the UNCLAMPED sample) and A = (adv[row] - adv_shift) * adv_scale:
 *
 *     mu = MLP(x)                                       atc_rollout_policy's arithmetic, the float64 first layer included (a wavefront of 64
 *                                                       consecutive rows i that holds a participating input above 4 in magnitude takes it)
 *     sigma_c = expf(log_std_c);  d_c = (u_c - mu_c) / sigma_c
 *     logp  = sum_c (-0.5 d_c^2 - log_std_c) - 1.5 log(2 pi)
 *     ratio = expf(logp - logp_old[row])
 *     L     = -min(ratio * A, clamp(ratio, 1 - clip, 1 + clip) * A)
 *     the gradient flows through the unclipped term iff (A >= 0 and ratio <= 1 + clip) or (A < 0 and ratio >= 1 - clip), and is zero
 *     otherwise (the row is CUT): what autograd yields for minimum(ratio A, clamp(ratio, 1 - clip, 1 + clip) A), boundaries inclusive
 *     dL/dlogp = -A ratio where it flows;  dlogp/dmu_c = d_c / sigma_c;  dlogp/dlog_std_c = d_c^2 - 1;  backpropagation through the two
 *     tanh layers
 *
 * OUTPUTS, with n the number of participating rows:
 *   grad   [ATC_POLICY_TRAFFIC_WORDS(K)], laid out like w: the sum of dL/dw over the participating rows, divided by n; all zeros if n == 0.
 *   stats  [ATC_PPO_GRAD_STATS] (the ATC_PPO_STAT_* words): n; mean L; mean (logp_old - logp), the approximate KL; the fraction of
 *          participating rows that were cut; mean ratio; max |logp - logp_old|; two reserved zeros.  All zeros if n == 0.
 *   logp_new [R], nullable: logp of row i, written for participating rows only; the others keep what they hold.
 *   scratch [G][ATC_POLICY_TRAFFIC_WORDS(K) + ATC_PPO_GRAD_STATS] floats, required: the G partial sums, overwritten by every call.
 * WORKGROUPS AND DETERMINISM.  G workgroups of one wavefront each take the tiles of 64 consecutive rows i in turn (workgroup g: tiles g,
 * g + G, ...).  workgroups == 0: G = min(number of tiles, ATC_PPO_GRAD_DEFAULT_WG); otherwise G = workgroups, 1 .. ATC_PPO_GRAD_MAX_WG.  No
 * floating-point atomics: a workgroup adds its rows in row order, the G partial sums are added in the order of g in float64 and rounded
 * once, and the division by n comes last.  The same inputs and the same G give the same bits on every run; another G gives another
 * rounding of the same sums.  One call is two launches on `stream`.
 * NOT IN THE CALL: the value loss and the critic — atc_ppo_value_grad and atc_value_forward below —; the trainer's: the entropy bonus —
 * with a log_std that does not depend on the state it is sum_c log_std_c + a constant, three words —, advantage normalisation (the trainer
 * passes its two scalars), and the optimiser.
 * ATC_ERR_ARG, in this order, atc_last_error() naming the argument: a NULL among s, w, obs_rows, action, logp_old, adv, g, out, out->grad,
 * out->stats, out->scratch; traffic_k outside {0, 1, 2, 4}; R_src < 1, R < 1, or index == NULL with R != R_src; clip not finite or <= 0;
 * workgroups outside 0 .. ATC_PPO_GRAD_MAX_WG; traffic NULL with traffic_k > 0, or given with traffic_k == 0; an output (grad, stats,
 * logp_new, scratch) sharing a byte with any other array of the call — pointer values only, ranges that only touch are accepted.
 * Counted by atc_ppo_policy_grad_launch_counts only: one count per CALL, slot = {0, 1, 2, 3 for traffic_k = 0, 1, 2, 4}. */
#define ATC_PPO_GRAD_MAX_WG 1024
#define ATC_PPO_GRAD_DEFAULT_WG 512
#define ATC_PPO_GRAD_STATS 8
#define ATC_PPO_STAT_N 0          /* participating rows */
#define ATC_PPO_STAT_LOSS 1       /* mean L */
#define ATC_PPO_STAT_KL 2         /* mean (logp_old - logp) */
#define ATC_PPO_STAT_CUT 3        /* fraction of participating rows whose gradient was cut */
#define ATC_PPO_STAT_RATIO 4      /* mean ratio */
#define ATC_PPO_STAT_DLOGP_MAX 5  /* max |logp - logp_old| */
typedef struct atc_ppo_grad {
    int32_t  traffic_k;   /* K: 0, 1, 2 or 4 */
    float    clip;        /* > 0, finite */
    float    adv_shift;   /* A = (adv - adv_shift) * adv_scale */
    float    adv_scale;
    int32_t  workgroups;  /* 0: the library's choice; else G = 1 .. ATC_PPO_GRAD_MAX_WG */
    uint32_t _pad;
} atc_ppo_grad_t;
typedef struct atc_ppo_grad_out {
    float* grad;      /* [ATC_POLICY_TRAFFIC_WORDS(K)] required */
    float* stats;     /* [ATC_PPO_GRAD_STATS] required */
    float* logp_new;  /* [R] nullable */
    float* scratch;   /* [G][ATC_POLICY_TRAFFIC_WORDS(K) + ATC_PPO_GRAD_STATS] required */
} atc_ppo_grad_out_t;
int atc_ppo_policy_grad(const atc_scenario_t* s, int R_src, int R, const float* w /* [ATC_POLICY_TRAFFIC_WORDS(K)] */,
                        const float* obs_rows /* [R_src][10] */, const float* traffic /* [R_src][K][8], with K > 0 */,
                        const float* action /* [R_src][3] */, const float* logp_old /* [R_src] */, const float* adv /* [R_src] */,
                        const uint8_t* mask /* nullable [R_src] */, const int32_t* index /* nullable [R] */,
                        const atc_ppo_grad_t* g, const atc_ppo_grad_out_t* out, void* stream);
enum { ATC_PPO_GRAD_LAUNCH_SLOTS = 4 };
int atc_ppo_policy_grad_launch_counts(uint64_t* out, int n);

/* THE CRITIC (extension): a value network with the policy's trunk and packing, evaluated and differentiated inside the library.
 * THE PACKED CRITIC.  One float32 array of ATC_VALUE_WORDS(K) words, IN = ATC_POLICY_TRAFFIC_IN(K) = 10 + 7 K:
 *     W1[64][IN], b1[64], W2[64][64], b2[64], W3[1][64], b3[1]          every matrix row-major [out][in]
 * — atc_policy_traffic_t.w without the two further rows of its head and without log_std.  V(x) = b3 + W3 tanh(b2 + W2 tanh(b1 + W1 x)).
 * It reads the input row of the policy: the own observation row, then words 0..6 of K traffic records.
 *
 * atc_value_forward: V of R rows in one launch.  x [R][IN] holds the rows already widened and contiguous (with K = 0: plain observation
 * rows); values [R] receives one word per row; no activation is written to memory.  All pointers are device pointers; `s` names the device
 * only.  ARITHMETIC, in fp32: atc_rollout_policy's for the hidden layers, in its operation order — layer 1 an fmaf chain over the inputs
 * starting from the bias, summed in float64 where a wavefront (64 consecutive rows, row 0 first) holds an input above 4 in magnitude, or a
 * NaN; layer 2 in four partial sums —, then v = b3; v = fmaf(W3[j], h2_j, v) for j = 0 .. 63.
 * ATC_ERR_ARG, in this order: a NULL among s, w, x, values; R < 1; traffic_k outside {0, 1, 2, 4}; values sharing a byte with x or w.
 * Counted by atc_value_forward_launch_counts only: slot = {0, 1, 2, 3 for traffic_k = 0, 1, 2, 4}. */
#define ATC_VALUE_WORDS(K) (4289 + 64 * ATC_POLICY_TRAFFIC_IN(K))   /* 4929, 5377, 5825, 6721 for K = 0, 1, 2, 4 */
int atc_value_forward(const atc_scenario_t* s, int R, int traffic_k, const float* w /* [ATC_VALUE_WORDS(K)] */,
                      const float* x /* [R][10 + 7 K] */, float* values /* [R] */, void* stream);
enum { ATC_VALUE_FORWARD_LAUNCH_SLOTS = 4 };
int atc_value_forward_launch_counts(uint64_t* out, int n);

/* PPO VALUE GRADIENT (extension): the value half of a PPO update in one call — the clipped value loss of the packed critic on stored
 * decisions and its gradient with respect to every word of w, summed over the rows of a minibatch.  With atc_ppo_policy_grad an update
 * touches no autograd: what is left to the trainer is the optimiser step on the two packed arrays (and the entropy bonus and advantage
 * normalisation named there).  No activation is written to global memory.
 * ROWS, INPUT ROW: atc_ppo_policy_grad's, word for word — R_src source rows read in place (obs_rows [R_src][10], traffic [R_src][K][8]),
 * R rows to evaluate through the nullable index, mask = atc_rollout_policy_ends' control; a row that does not participate loads nothing
 * but its index and mask byte and is taken out by selects: a NaN standing in it changes no output bit.
 * PER PARTICIPATING ROW, in fp32, with v = V(x) in atc_value_forward's arithmetic (a wavefront = the 64 consecutive rows i of a tile, the
 * rows that do not participate counting as zeros):
 *
 *     e = v - ret;  d = v - v_old;  vc = v_old + clamp(d, -clip, +clip);  ec = vc - ret
 *     |d| <= clip (always so with clip = +inf):  L = 0.5 e^2,   dL/dv = e
 *     otherwise, e^2 >= ec^2:                    L = 0.5 e^2,   dL/dv = e
 *     otherwise the row is CUT:                  L = 0.5 ec^2,  dL/dv = 0
 *
 * — PPO2's 0.5 max((v - ret)^2, (vc - ret)^2), with the one gradient autograd's maximum has away from a tie.  A NaN v is not cut: it stays
 * a NaN in L, in the gradient and in value.  Backpropagation through the two tanh layers as in atc_ppo_policy_grad.
 * OUTPUTS, with n the number of participating rows:
 *   grad   [ATC_VALUE_WORDS(K)], laid out like w: the sum of dL/dw over the participating rows, divided by n; all zeros if n == 0.
 *   stats  [ATC_PPO_VALUE_STATS] (the ATC_PPO_VSTAT_* words): n; mean L; the fraction of participating rows that were cut; mean v; mean
 *          ret; mean ret^2; mean (ret - v)^2; max |v - v_old|.  Words 4 .. 6 give the explained variance 1 - mean (ret - v)^2 /
 *          (mean ret^2 - (mean ret)^2) without another pass.  All zeros if n == 0.
 *   value  [R], nullable: v of row i, written for participating rows only; the others keep what they hold.  Where the tiles of 64 rows
 *          hold the same rows (those that do not participate as zeros), it equals atc_value_forward's output bit for bit.
 *   scratch [G][ATC_VALUE_WORDS(K) + ATC_PPO_VALUE_STATS] floats, required: the G partial sums, overwritten by every call.
 * WORKGROUPS AND DETERMINISM: atc_ppo_policy_grad's (the same default, the same maximum, no atomics, float64 in the order of g, the
 * division by n last).  One call is two launches on `stream`.
 * ATC_ERR_ARG, in this order: a NULL among s, w, obs_rows, v_old, ret, g, out, out->grad, out->stats, out->scratch; traffic_k outside
 * {0, 1, 2, 4}; R_src < 1, R < 1, or index == NULL with R != R_src; clip NaN or <= 0 (+inf is the plain squared error); workgroups outside
 * 0 .. ATC_PPO_GRAD_MAX_WG; traffic NULL with traffic_k > 0, or given with traffic_k == 0; an output (grad, stats, value, scratch) sharing
 * a byte with any other array of the call.
 * Counted by atc_ppo_value_grad_launch_counts only: one count per CALL, slot = {0, 1, 2, 3 for traffic_k = 0, 1, 2, 4}. */
#define ATC_PPO_VALUE_STATS 8
#define ATC_PPO_VSTAT_N 0        /* participating rows */
#define ATC_PPO_VSTAT_LOSS 1     /* mean L */
#define ATC_PPO_VSTAT_CUT 2      /* fraction of participating rows whose gradient was cut */
#define ATC_PPO_VSTAT_V 3        /* mean v */
#define ATC_PPO_VSTAT_RET 4      /* mean ret */
#define ATC_PPO_VSTAT_RET2 5     /* mean ret^2 */
#define ATC_PPO_VSTAT_ERR2 6     /* mean (ret - v)^2 */
#define ATC_PPO_VSTAT_DV_MAX 7   /* max |v - v_old| */
typedef struct atc_ppo_value_grad {
    float    clip;        /* > 0; +inf: no clipping */
    int32_t  workgroups;  /* 0: the library's choice; else G = 1 .. ATC_PPO_GRAD_MAX_WG */
} atc_ppo_value_grad_t;
typedef struct atc_ppo_value_grad_out {
    float* grad;      /* [ATC_VALUE_WORDS(K)] required */
    float* stats;     /* [ATC_PPO_VALUE_STATS] required */
    float* value;     /* [R] nullable */
    float* scratch;   /* [G][ATC_VALUE_WORDS(K) + ATC_PPO_VALUE_STATS] required */
} atc_ppo_value_grad_out_t;
int atc_ppo_value_grad(const atc_scenario_t* s, int R_src, int R, int traffic_k, const float* w /* [ATC_VALUE_WORDS(K)] */,
                       const float* obs_rows /* [R_src][10] */, const float* traffic /* [R_src][K][8], with K > 0 */,
                       const float* v_old /* [R_src] */, const float* ret /* [R_src] */,
                       const uint8_t* mask /* nullable [R_src] */, const int32_t* index /* nullable [R] */,
                       const atc_ppo_value_grad_t* g, const atc_ppo_value_grad_out_t* out, void* stream);
enum { ATC_PPO_VALUE_GRAD_LAUNCH_SLOTS = 4 };
int atc_ppo_value_grad_launch_counts(uint64_t* out, int n);

/* ADVANTAGE NORMALISATION (extension): mean and standard deviation of the advantages of a collection and the normalised advantages, in two
 * launches on `stream` with no host read.  `s` names the device only; all array pointers are device pointers.
 * ROWS.  adv [R] float32.  Row r PARTICIPATES if mask is NULL or mask[r] != 0 (atc_rollout_policy_ends' control, flattened); a row that
 * does not is not read: a NaN standing there changes no output bit.
 * LAUNCH 1.  G workgroups of ATC_ADV_TILE = 256 lanes; workgroup g takes the tiles of 256 consecutive rows g, g + G, ...  Lane l adds its row
 * of each tile, in tile order, into float64 accumulators: n += 1; S += a; S2 += a * a (the product in float64).  Lane 0 adds the 256 lanes'
 * triples in lane order 0 .. 255 and writes scratch[g] = {n, S, S2}.
 * LAUNCH 2.  Every workgroup adds the G triples in the order of g in float64, then
 *     mean = S / n;  var = max(0, S2 - S * mean) / (n - 1), 0 with n == 1 (the unbiased form, torch.std's);  std = sqrt(var)
 *     shift = (float)mean;  scale = (float)(1.0 / (std + (double)eps))
 *     out_adv[r] = (adv[r] - shift) * scale in float32 for a participating row — atc_ppo_policy_grad's A = (adv - adv_shift) * adv_scale
 *     word for word, so that call gives the same bits on (out_adv, 0, 1) as on (adv, stats[MEAN], stats[SCALE]) — and 0.0f, by a select,
 *     for a row that takes no part.
 * stats [ATC_ADV_STATS] = {n, shift, scale, (float)std} (the ATC_ADV_STAT_* words).  With n == 0, stats and out_adv are all zeros.
 * out_adv is nullable, and may be adv itself (in place: equal pointers); no other output may share a byte with another array of the call.
 * scratch [G][3] doubles, required, overwritten by every call.  workgroups == 0: G = min(tiles, ATC_ADV_DEFAULT_WG); otherwise G =
 * workgroups, 1 .. ATC_ADV_MAX_WG.  No atomics: the same inputs and the same G give the same bits on every run.
 * NUMERICAL LIMIT.  S and S2 are plain float64 moments: the variance loses accuracy as |mean| / std approaches 1e7 (the difference
 * S2 - S * mean cancels about 2 log10(|mean| / std) of float64's 16 digits).  Advantages are nowhere near that.
 * ATC_ERR_ARG, in this order: a NULL among s, adv, g, out, out->stats, out->scratch; R < 1; eps not finite or < 0; workgroups outside
 * 0 .. ATC_ADV_MAX_WG; an output sharing a byte with another array (out_adv == adv excepted).
 * Counted by atc_adv_normalise_launch_counts only: one slot, one count per CALL. */
#define ATC_ADV_TILE 256
#define ATC_ADV_MAX_WG 1024
#define ATC_ADV_DEFAULT_WG 256
#define ATC_ADV_STATS 4
#define ATC_ADV_STAT_N 0       /* participating rows */
#define ATC_ADV_STAT_MEAN 1    /* shift: the mean, rounded to float32 */
#define ATC_ADV_STAT_SCALE 2   /* scale: 1 / (std + eps), rounded to float32 */
#define ATC_ADV_STAT_STD 3     /* the standard deviation, rounded to float32 */
typedef struct atc_adv_norm {
    float    eps;         /* >= 0, finite */
    int32_t  workgroups;  /* 0: the library's choice; else G = 1 .. ATC_ADV_MAX_WG */
} atc_adv_norm_t;
typedef struct atc_adv_norm_out {
    float*  out_adv;   /* [R] nullable; may be adv */
    float*  stats;     /* [ATC_ADV_STATS] required */
    double* scratch;   /* [G][3] required */
} atc_adv_norm_out_t;
int atc_adv_normalise(const atc_scenario_t* s, int R, const float* adv /* [R] */, const uint8_t* mask /* nullable [R] */,
                      const atc_adv_norm_t* g, const atc_adv_norm_out_t* out, void* stream);
enum { ATC_ADV_NORMALISE_LAUNCH_SLOTS = 1 };
int atc_adv_normalise_launch_counts(uint64_t* out, int n);

/* ADAM STEP (extension): PPO2's optimiser step on one or two packed tensors (the policy and the critic) in ONE launch of one workgroup —
 * the global gradient-norm clip over both, the entropy term on log_std, and Adam.  `s` names the device only.
 * EFFECTIVE GRADIENT of word i of tensor k, in float64:
 *     ge = (double)grad_scale * (double)grad[i] + (add_first <= i < add_first + add_count ? (double)add_value : 0)
 * grad_scale is vf_coef for the critic.  The add window carries the entropy bonus: the entropy of the diagonal Gaussian is sum log_std + a
 * constant, so -ent_coef * H adds exactly -ent_coef to each of the three log_std words (add_first = their offset, add_count = 3,
 * add_value = -ent_coef).
 * THE WORKGROUP.  ATC_ADAM_BLOCK = 1 024 lanes over the concatenated index j (tensor 0's words, then tensor 1's).  Lane l adds ge * ge over
 * j = l, l + 1024, ... in float64; lane 0 adds the 1 024 sums in lane order; norm = sqrt(total);
 *     coef = (max_norm > 0 and max_norm < inf) ? min(1, max_norm / (norm + 1e-6)) : 1          (torch.nn.utils.clip_grad_norm_'s rule)
 * then every word, in float64, each stored word rounded to float32 exactly once, with c1 = 1 - beta1^step and c2 = 1 - beta2^step made on
 * the host in double:
 *     gc = ge * coef
 *     m' = (float)(beta1 * m + (1 - beta1) * gc)
 *     v' = (float)(beta2 * v + ((1 - beta2) * gc) * gc)
 *     w' = (float)(w - (lr / c1) * (m' / (sqrt(v') / sqrt(c2) + eps)))          with the ROUNDED m' and v' that are stored
 * — torch.optim.Adam's step (no weight decay, no amsgrad) in its operation order.  No product is fused with a sum.  Float64 with one
 * rounding per stored word makes the result independent of how float32 division and square root are lowered.
 * NON-FINITE GRADIENTS.  If norm is not finite, nothing is written to w, m or v.
 * stats [ATC_ADAM_STATS] = {(float)norm, (float)coef (0 where skipped), skipped (0 / 1), (float)step}.
 * ATC_ERR_ARG, in this order: a NULL among s, t, g, stats; n_tensors not 1 or 2; per tensor a NULL among w, grad, m, v; words outside
 * 1 .. ATC_ADAM_MAX_WORDS; add_count < 0, or add_count > 0 with the window outside the tensor; grad_scale or add_value not finite;
 * step < 1; lr, eps or a beta not finite, lr < 0, eps < 0, a beta outside [0, 1); max_norm a NaN; any two of w, grad, m, v of both
 * tensors and stats sharing a byte.
 * Counted by atc_adam_step_launch_counts only: slot = n_tensors - 1. */
#define ATC_ADAM_BLOCK 1024
#define ATC_ADAM_MAX_WORDS 65536
#define ATC_ADAM_STATS 4
#define ATC_ADAM_STAT_NORM 0      /* the norm of the effective gradient over all tensors */
#define ATC_ADAM_STAT_COEF 1      /* the clip coefficient applied (1: not clipped) */
#define ATC_ADAM_STAT_SKIPPED 2   /* 1 where the norm was not finite and nothing was written */
#define ATC_ADAM_STAT_STEP 3      /* step, as passed */
typedef struct atc_adam_tensor {
    float*       w;            /* [words] updated in place */
    const float* grad;         /* [words] */
    float*       m;            /* [words] first moment, updated in place */
    float*       v;            /* [words] second moment, updated in place */
    int32_t      words;        /* 1 .. ATC_ADAM_MAX_WORDS */
    float        grad_scale;
    int32_t      add_first;
    int32_t      add_count;    /* 0: no window */
    float        add_value;
} atc_adam_tensor_t;
typedef struct atc_adam {
    double  lr;
    double  beta1;
    double  beta2;
    double  eps;
    double  max_norm;   /* <= 0 or +inf: no clip */
    int32_t step;       /* >= 1 */
} atc_adam_t;
int atc_adam_step(const atc_scenario_t* s, int n_tensors /* 1 or 2 */, const atc_adam_tensor_t* t /* [n_tensors] */, const atc_adam_t* g,
                  float* stats /* [ATC_ADAM_STATS] */, void* stream);
enum { ATC_ADAM_STEP_LAUNCH_SLOTS = 2 };
int atc_adam_step_launch_counts(uint64_t* out, int n);

/* POLICY FORWARD (extension): the decisions of the packed policy on given rows, OUTSIDE a rollout — what deployment (observation ->
 * decision -> step -> render), a planner that seeds its candidates from the policy, or any other consumer of a trained policy needs without
 * restating the MLP.  The critic's atc_value_forward with the policy's head and its draw.  A pure function of its arrays: `s` names the
 * device only; all pointers are device pointers.
 * INPUT ROW: atc_ppo_policy_grad's — obs_rows[r][0..9], then words 0..6 of each of the K = traffic_k records traffic[r][k][0..7] (word 7 is
 * not read): what atc_rollout_policy_traffic stores and what atc_observe_traffic writes, read in place.  w is the packed policy,
 * ATC_POLICY_TRAFFIC_WORDS(K) floats.
 * ARITHMETIC, in fp32: atc_rollout_policy's, in its operation order — layer 1 an fmaf chain over the inputs starting from the bias, summed in
 * float64 where a wavefront (64 consecutive rows, row 0 first) holds an input above 4 in magnitude, or a NaN; layer 2 in four partial sums;
 * mu_c = b3_c, then mu_c = fmaf(W3[c][j], h2_j, mu_c) for j = 0 .. 63.  The MLP is evaluated ONCE per row.  Then, for sample s = 0 .. S - 1
 * of row r, with P = rows_per_decision (0 means R) and DS = ceil(R / P):
 *
 *     decision = decision0 + s * DS + r / P   (modulo 2^32);   i = r % P
 *     key = mix64( mix64(seed ^ (u64)decision) ^ (u64)i );  z_c, u_c, a_c and logp as in atc_rollout_policy
 *
 * With S = 1 and P = B * N, the rows [D][B][N] that a rollout's decisions saw get exactly the rollout's keys; further samples continue the
 * decision counter behind them, so no two samples of one call share a key.
 * BIT EQUALITY WITH THE ROLLOUT holds for a row whose wavefront takes the same form of layer 1 here and there: the rollout's wavefront is 64
 * consecutive lane slots of its launch, this call's is 64 consecutive rows.  Where the two may choose differently (an input above 4 in
 * one's wavefront and not in the other's), the claim is the bars of tests/policy_ref.py, not bit equality.
 * OUTPUTS, each nullable, at least one given: mean [R][3] = mu; action [S][R][3] = u, the UNCLAMPED sample (atc_policy_out_t.action);
 * flown [S][R][3] = a, its clamp to [-1, 1], what a step is to be given (a NaN gives -1); logp [S][R].  ATC_POLICY_DETERMINISTIC: u = mu,
 * logp = 0, no key is evaluated; S must be 1.
 * ATC_ERR_ARG, in this order, atc_last_error() naming the argument: a NULL among s, w, obs_rows, f, out; traffic_k outside {0, 1, 2, 4};
 * R < 1; samples outside 1 .. ATC_POLICY_FWD_MAX_SAMPLES, or rows_per_decision outside 0 .. R; ATC_POLICY_DETERMINISTIC with samples > 1;
 * unknown flag bits; traffic NULL with traffic_k > 0, or given with traffic_k == 0; every output NULL; an output sharing a byte with any
 * other array of the call — pointer values only, ranges that only touch are accepted.
 * Counted by atc_policy_forward_launch_counts only: slot = {0, 1, 2, 3 for traffic_k = 0, 1, 2, 4}; one launch per call. */
enum { ATC_POLICY_FWD_MAX_SAMPLES = 64 };
typedef struct atc_policy_fwd {
    int32_t  traffic_k;          /* K: 0, 1, 2 or 4 */
    int32_t  samples;            /* S: 1 .. ATC_POLICY_FWD_MAX_SAMPLES */
    int32_t  rows_per_decision;  /* P: 1 .. R; 0 means R */
    uint32_t flags;              /* ATC_POLICY_DETERMINISTIC or 0 */
    uint64_t seed;
    uint32_t decision0;          /* number of the decision rows 0 .. P - 1 of sample 0 belong to */
    uint32_t reserved;
} atc_policy_fwd_t;
typedef struct atc_policy_fwd_out {
    float* mean;     /* [R][3]    nullable */
    float* action;   /* [S][R][3] nullable: the UNCLAMPED sample u */
    float* flown;    /* [S][R][3] nullable: fminf(fmaxf(u, -1), 1) */
    float* logp;     /* [S][R]    nullable */
} atc_policy_fwd_out_t;
int atc_policy_forward(const atc_scenario_t* s, int R, const float* w /* [ATC_POLICY_TRAFFIC_WORDS(K)] */,
                       const float* obs_rows /* [R][10] */, const float* traffic /* [R][K][8], with K > 0 */,
                       const atc_policy_fwd_t* f, const atc_policy_fwd_out_t* out, void* stream);
enum { ATC_POLICY_FORWARD_LAUNCH_SLOTS = 4 };
int atc_policy_forward_launch_counts(uint64_t* out, int n);

/* POLICY LOOK-AHEAD (extension): atc_lookahead_plan whose candidates are CONTINUED BY THE POLICY inside the launch — "if I take this
 * decision now and then go on as I would, how does it end?" for M candidates per env in ONE launch that writes no state and no per-step
 * stream: what an action shield, a Monte-Carlo estimate of Q(s, a) / V(s) and the tail value of a planner ask.  1 <= K <= ATC_SKIP_MAX,
 * 1 <= H <= ATC_PLAN_MAX_H, 1 <= M <= ATC_SAMPLE_MAX_M; pol is the ten-word policy of atc_rollout_policy (a traffic policy is not taken).
 * Candidate m of env e is a bit-exact private copy of the env's state; segment h = 0 .. H-1 holds ONE decision for K steps.
 *   first != NULL ([M][B*N*3], clamped actions as atc_lookahead takes them): segment 0 flies first[m], the policy decides segments
 *                 1 .. H-1, h0 = 1; obs0 is not read and may be NULL.
 *   first == NULL: the policy decides every segment, h0 = 0; segment 0 sees obs0 ([B*N*10], as in atc_rollout_policy), the same rows for
 *                 every candidate — the candidates then differ by their draws alone.
 * The decision of segment h >= h0 is atc_rollout_policy's (h1, h2, mu, key, z, u, a, logp as defined there) on the ten words the previous
 * step of THAT candidate stored, with
 *
 *     decision = pol->decision0 + (h - h0)   (modulo 2^32);     i = (m*B + e)*N + k
 *
 * which is the key atc_rollout_policy(seed, decision0) uses on a child batch of M*B envs whose env m*B + e is the candidate — atc_branch's
 * numbering.  The call therefore EQUALS, in every output, a composition of existing calls on such a child (tests/lookahead_policy_ref.py
 * folds its [T][M*B] arrays): atc_state_select(index = c % B) then atc_rollout_policy(H*K, hold = K, obs0 tiled M times) where first is NULL;
 * atc_branch(first, K) then atc_rollout_policy((H-1)*K, hold = K, obs0 = the branch's obs) where it is given — each candidate cut at its
 * first done.  BIT FOR BIT wherever no wavefront of either side sums layer 1 in float64 (atc_policy_forward: an input above 4 in
 * magnitude, or a NaN, in the wavefront; here a lane whose env has taken its last step feeds zeros and never switches its wavefront).
 * Normalised observations lie in [-1, 1]; what exceeds 4 is an unnormalised observation and the raw reset observation that follows an
 * auto-reset in the CHILD's rollout.  Where the two sides choose differently the policy half is held to the bars of tests/policy_ref.py
 * at the first affected decision, as for atc_policy_forward, and what follows it is that of the decision taken.
 * Everything else is atc_lookahead_plan's contract, word for word: an env stops at its first done, so a plan never spans two episodes; the
 * segments it did not run get seg_reward 0; reward and ac_reward are the two-level sequential fp32 sums; flags the OR, min_sep the minimum,
 * obs the last executed step's; the WIDE-heading rule (n_steps = 0 and every word of atc_plan_out_t's arrays zero for that (m, e)); no
 * state written.  Two additions, each nullable:
 *   flown [M][H][B*N*3]  the clamped action segment h flew (first[m] in segment 0 where given).  Rows of segments an env did not run are
 *                        left alone.  flown[.][0] is what atc_step_skip takes to execute a winner when first was NULL.
 *   logp  [M][H][B*N]    written for the segments the policy decided and the env ran (0 under ATC_POLICY_DETERMINISTIC).
 * (A not-evaluated (m, e) keeps the flown / logp rows written before its WIDE heading was seen; n_steps == 0 tells.)
 * ATC_ERR_ARG, in this order, atc_last_error() naming the argument: a NULL among pol, pol->w, out, out->reward, out->done, obs0 where first
 * is NULL, then s, st, p and st's six arrays; K outside 1 .. ATC_SKIP_MAX; H outside 1 .. ATC_PLAN_MAX_H; M outside 1 .. ATC_SAMPLE_MAX_M;
 * ATC_M_DISCRETE, then ATC_M_ACTIONS_HELD in p->mode; pol->n_hidden != ATC_POLICY_HIDDEN or unknown bits in pol->flags; B or N out of
 * range, B*N too large for a launch, M*B*N >= 2^32; pol->w overlapping an output; an output overlapping any other array of the call
 * (obs0, first, st's arrays, another output) — pointer values only, ranges that only touch are accepted; dt out of range (atc_step's rule).
 * Counted by atc_lookahead_policy_launch_counts only (slot = log2(W); the rules of atc_skip_launch_counts): every other launch record
 * stays still, and a refused call moves none.  atc_lookahead_set_mapping governs this call's candidates per workgroup as well; results
 * do not depend on it. */
typedef struct atc_lookahead_policy_out {
    float*    reward;     /* [M][B]        required */
    uint8_t*  done;       /* [M][B]        required */
    uint16_t* n_steps;    /* [M][B]        nullable; total executed steps (<= H*K = 4080); 0 = not evaluated */
    float*    seg_reward; /* [M][H][B]     nullable */
    uint16_t* flags;      /* [M][B*N]      nullable */
    float*    ac_reward;  /* [M][B*N]      nullable */
    float*    min_sep;    /* [M][B]        nullable */
    float*    obs;        /* [M][B*N*10]   nullable */
    float*    flown;      /* [M][H][B*N*3] nullable */
    float*    logp;       /* [M][H][B*N]   nullable */
} atc_lookahead_policy_out_t;
int atc_lookahead_policy(const atc_scenario_t* s, int B, int N, int K, int H, int M, const atc_state_t* st,
                         const float* obs0 /* [B*N*10]; nullable where first is given */, const float* first /* nullable [M][B*N*3] */,
                         const atc_policy_t* pol, const atc_lookahead_policy_out_t* out, const atc_params_t* p, void* stream);
enum { ATC_LOOKAHEAD_POLICY_LAUNCH_SLOTS = 7 };
int atc_lookahead_policy_launch_counts(uint64_t* out, int n);

#ifdef __cplusplus
}
#endif
#endif /* ATC_STEP_H */
