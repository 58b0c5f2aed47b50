"""Word layout of the scenario blob and flag/mode bits — Python mirror of include/atc_step.h.

tests/test_abi.py parses the header and checks that every constant here matches it.
"""
ABI_VERSION = 22
BLOB_VERSION = 1014.0

H_VERSION, H_NWORDS, H_N_MVA, H_N_NOISE, H_N_ENTRY, H_OFF_POLY, H_OFF_VERT, H_OFF_ENTRY, H_OFF_GRID, H_N_VERTW = range(10)
H_OFF_SLOT = 10
H_OFF_SPAWN = 11
SPAWN_WORDS = 16
C_RWY_X, C_RWY_Y, C_RWY_H, C_PHI_TO_RWY, C_FAF_X, C_FAF_Y, C_NRM_X, C_NRM_Y = range(16, 24)
C_FAF_ANGLE, C_GS_TAN, C_FAF_MVA, C_WORLD_DIAG, C_NM_TO_FT = range(24, 29)
C_V_MIN, C_V_MAX, C_H_MIN, C_H_MAX, C_A_MIN, C_A_MAX, C_HDOT_MIN, C_HDOT_MAX = range(29, 37)
C_PHIDOT_MIN, C_PHIDOT_MAX, C_V_INIT = 37, 38, 39
C_TRI_H, C_TRI_1, C_TRI_2 = 40, 48, 56
C_NORM_MIN, C_NORM_MAX, C_ACT_DISCR, C_BBOX = 64, 74, 84, 87
C_DIR_RWY_X, C_DIR_RWY_Y = 91, 92
C_ALIGNED_OK = 93
C_POS_X0, C_POS_Y0, C_POS_SCALE, C_POS_INV = 94, 95, 100, 101   # fixed-point position grid: nm = X0 + fix * 2^-k
C_FAF_FIX = 124                                                 # FAF on the grid: x (hi, lo), y (hi, lo); fix = hi * 65536 + lo
POS_MAX_K = 27
# speed / heading state: 32-bit fixed point (include/atc_step.h, ABI 18; the heading field saturates since ABI 19: below): kt = v_fix 2^-23 (unsigned), deg = 180 + phi_fix 2^-23
V_FIX_SHIFT, PHI_FIX_SHIFT, PHI_FIX_OFFSET = 23, 23, 180.0
# ABI 19: the heading is unbounded like the reference's (model.py:104-120) — a 32-bit field that SATURATES (INT32_MIN / INT32_MAX =
# "WIDE") in front of the exact integer-valued float64 counts in atc_state_t.phi_wide[i][0] ([1]: the last heading target)
PHI_WIDE_WORDS = 4
PHI_LIMIT = 2.0 ** 52
I32_MIN, I32_MAX = -2 ** 31, 2 ** 31 - 1
C_TRI_BBOX = 96
C_NORM_A, C_NORM_B = 104, 114
C_END = 128

P_MINX, P_MINY, P_MAXX, P_MAXY, P_HEIGHT, P_VOFF, P_NVERT, P_PENALTY, P_WORDS = range(9)
E_X, E_Y, E_PHI, E_NLEV, E_LEV0 = range(5)
E_WORDS, E_MAXLEV = 12, 8
G_X0, G_Y0, G_INV, G_NX, G_NY, G_OFF_POOL, G_NREC = range(7)
G_HDR = 8
GE_WORDS = 8

PKT_CHUNKS = 9
MAX_AIRCRAFT = 64
OBS_DIM = 10
ACT_DIM = 3

F_BELOW_MVA, F_OUTSIDE, F_WON, F_TIMEOUT = 1, 2, 4, 8
F_INVALID_V, F_INVALID_H, F_CONFLICT, F_NOISE, F_INACTIVE, F_PHI_LIMIT = 16, 32, 64, 128, 256, 512
F_TERMINAL = F_BELOW_MVA | F_OUTSIDE | F_TIMEOUT | F_CONFLICT  # episode-ending on their own (WON: when all handed over)

M_REWARD_SHAPING, M_NORMALIZE, M_DISCRETE, M_AUTO_RESET, M_RANDOM_ENTRY, M_KEEP_ACTIVE, M_ACTIONS_HELD = 1, 2, 4, 8, 16, 32, 64

# per-step env record (atc_state_t.env): 4 x 32-bit words, float fields by bit pattern
ENV_TIMESTEPS, ENV_ACTIONS_TAKEN, ENV_TOTAL_REWARD, ENV_MASK_LO, ENV_WORDS = range(5)
# per-episode env record (atc_state_t.stats): 8 x 32-bit words
STAT_EPISODES, STAT_EP_LENGTH, STAT_EP_RETURN, STAT_WIN_BITS, STAT_EP_ACTIONS, STAT_MASK_HI = range(6)
STAT_WORDS = 8
# aircraft record (atc_state_t.ac, 4 x int32): x / y position counts, heading counts, speed counts; atc_state_t.alt: float64 [ft];
# last-action record (atc_state_t.last_act, 4 x int32): speed counts, heading counts, altitude target float64 in words 2..3
AC_X, AC_Y, AC_PHI, AC_V, AC_WORDS = range(5)
LA_V, LA_PHI, LA_H, LA_WORDS = 0, 1, 2, 4
# LDS-resident lookup table (include/atc_step.h: ATC_LDS_*)
LDS_MAGIC = 0x3154444C
(LDS_H_MAGIC, LDS_H_BYTES, LDS_H_X0, LDS_H_Y0, LDS_H_INV, LDS_H_NX, LDS_H_NY, LDS_H_OFF_L1, LDS_H_OFF_SUB, LDS_H_N_SUB, LDS_H_OFF_LINE,
 LDS_H_N_LINE, LDS_H_OFF_HTS, LDS_H_SUB, LDS_H_OFF_RESID, LDS_H_N_RESID, LDS_H_LDS_BYTES, LDS_H_OFF_POOL, LDS_H_N_REC) = range(19)
LDS_HDR_WORDS = 24
LDS_CLEAN, LDS_LINE, LDS_SUB, LDS_RESID = 0, 1, 2, 3
# launch record (include/atc_step.h, ABI 22: atc_launch_counts): slot = log2(W) * LF_FORMS + form, LAUNCH_SERVE for server starts
LF_FULL_ONE, LF_FULL_MULTI, LF_GEN_ONE, LF_ALLV_ONE, LF_GEN_MULTI, LF_ALLV_MULTI, LF_LAT, LF_LDSG, LF_FORMS = range(9)
LAUNCH_SERVE, LAUNCH_SLOTS = 56, 57
LF_NAMES = ("full-one", "full-multi", "gen-one", "allv-one", "gen-multi", "allv-multi", "lat", "ldsg")
# frame skip (include/atc_step.h: atc_step_skip): largest block length; its own launch record, slot = log2(W)
SKIP_MAX, SKIP_LAUNCH_SLOTS = 255, 7
# traffic observation (include/atc_step.h: atc_observe_traffic): K <= TRAFFIC_MAX_K records of TRAFFIC_DIM words per aircraft; its own
# launch record, slot = log2(W)
TRAFFIC_DIM, TRAFFIC_MAX_K = 8, 8
T_PRESENT, T_DIST, T_AHEAD, T_RIGHT, T_DH, T_DV_AHEAD, T_DV_RIGHT, T_SLOT = range(8)
TRAFFIC_LAUNCH_SLOTS = 7
# what-if look-ahead (include/atc_step.h: atc_lookahead): at most LOOKAHEAD_MAX_M candidate action blocks per call; its own launch
# record (slot = log2(W))
LOOKAHEAD_MAX_M, LOOKAHEAD_LAUNCH_SLOTS = 64, 7
# plan look-ahead (include/atc_step.h: atc_lookahead_plan): at most PLAN_MAX_H held action blocks per candidate; its own launch
# record (slot = log2(W))
PLAN_MAX_H = 16
PLAN_LAUNCH_SLOTS = 7
# drawn plans (include/atc_step.h: atc_lookahead_plan_sampled, atc_plan_draw): at most SAMPLE_MAX_M candidates drawn inside the launch;
# DRAW_MEAN_FIRST: the flag of atc_plan_draw_t that makes candidate 0 the mean; DRAW_SCALE_BITS: the bit pattern of the fp32 factor of
# the draw (0x1.bb67aep-16); their own launch records (sampled: slot = log2(W); draw: one slot)
SAMPLE_MAX_M = 1024
DRAW_MEAN_FIRST = 1
DRAW_SCALE_BITS = 0x37DDB3D7
PLAN_SAMPLED_LAUNCH_SLOTS = 7
PLAN_DRAW_LAUNCH_SLOTS = 1
# the refit on drawn plans (include/atc_step.h: atc_plan_refit): its own launch record, one slot
PLAN_REFIT_LAUNCH_SLOTS = 1
# scoring and ranking of drawn plans (include/atc_step.h: atc_plan_score): at most SCORE_MAX_TOP rows of best candidate numbers; the two
# modes of atc_plan_score_t; its own launch record, one slot
SCORE_MAX_TOP = 64
SCORE_ELITE, SCORE_SOFTMAX = 0, 1
PLAN_SCORE_LAUNCH_SLOTS = 1
# branch and select (include/atc_step.h: atc_branch, atc_state_select): their own launch records (atc_branch_launch_counts: slot =
# log2(W); atc_select_launch_counts: one slot)
BRANCH_LAUNCH_SLOTS = 7
SELECT_LAUNCH_SLOTS = 1
# policy rollout (include/atc_step.h: atc_rollout_policy): the MLP is POLICY_IN -> POLICY_HIDDEN -> POLICY_HIDDEN -> ACT_DIM, POLICY_WORDS
# floats in one array (W1, b1, W2, b2, W3, b3, log_std; weights row-major [out][in]); POLICY_DETERMINISTIC: the flag of atc_policy_t that
# flies the mean; its own launch record (slot = log2(W))
POLICY_IN, POLICY_HIDDEN, POLICY_WORDS = 10, 64, 5062
POLICY_DETERMINISTIC = 1
ROLLOUT_POLICY_LAUNCH_SLOTS = 7
# policy rollout with traffic (include/atc_step.h: atc_rollout_policy_traffic): the first layer is policy_in(K) = 10 + 7 K wide — the own row,
# then words 0..6 of each of the K records — and the array policy_words(K) floats, laid out like POLICY_WORDS; K is one of POLICY_TRAFFIC_K; its
# own launch record (slot = 3 log2(W) + log2(K))
POLICY_TRAFFIC_K = (1, 2, 4)
POLICY_TRAFFIC_WORDS_PER_RECORD = 7
ROLLOUT_POLICY_TRAFFIC_LAUNCH_SLOTS = 21
# advantages and returns of a collection (include/atc_step.h: atc_gae): the two flags of atc_gae_t; at most GAE_MAX_NV value columns per env;
# its own launch record, one slot
GAE_PER_DECISION, GAE_REWARD_PER_COLUMN = 1, 2
GAE_MAX_NV = 64
GAE_LAUNCH_SLOTS = 1
# policy rollout with episode ends (include/atc_step.h: atc_rollout_policy_ends): TERM_ENDED is the bit of term_flags that says the block has
# an ending step (the flag bits of the env's aircraft at that step are OR-ed below it); its record counts by width and K in (0, 1, 2, 4).
# atc_gae_boot has one slot.
TERM_ENDED = 0x8000
ROLLOUT_POLICY_ENDS_LAUNCH_SLOTS = 28
GAE_BOOT_LAUNCH_SLOTS = 1
# policy rollout with terminal traffic records (include/atc_step.h: atc_rollout_policy_term): K in POLICY_TRAFFIC_K only; a record of its own,
# counted by width and K like the traffic rollout's (slot = 3 log2(W) + log2(K))
ROLLOUT_POLICY_TERM_LAUNCH_SLOTS = 21
# the PPO policy loss and gradient (include/atc_step.h: atc_ppo_policy_grad): at most PPO_GRAD_MAX_WG workgroups = partial rows of `scratch`,
# PPO_GRAD_DEFAULT_WG where the caller leaves the choice to the library; the words of `stats`; its record counts calls by K in (0, 1, 2, 4)
PPO_GRAD_MAX_WG = 1024
PPO_GRAD_DEFAULT_WG = 512
PPO_GRAD_TILE = 64
PPO_GRAD_STATS = 8
PPO_STAT_N, PPO_STAT_LOSS, PPO_STAT_KL, PPO_STAT_CUT, PPO_STAT_RATIO, PPO_STAT_DLOGP_MAX = range(6)
PPO_GRAD_LAUNCH_SLOTS = 4
# the critic (include/atc_step.h: atc_value_forward, atc_ppo_value_grad): the policy's trunk with one output, value_words(K) floats in one array
# (W1, b1, W2, b2, W3[1][64], b3[1]); the words of atc_ppo_value_grad's `stats`; both records count calls by K in (0, 1, 2, 4).  Workgroups and
# scratch rows are the policy gradient's (PPO_GRAD_MAX_WG, PPO_GRAD_DEFAULT_WG, ppo_grad_workgroups).
VALUE_WORDS = 4929
PPO_VALUE_STATS = 8
(PPO_VSTAT_N, PPO_VSTAT_LOSS, PPO_VSTAT_CUT, PPO_VSTAT_V, PPO_VSTAT_RET, PPO_VSTAT_RET2, PPO_VSTAT_ERR2, PPO_VSTAT_DV_MAX) = range(8)
VALUE_FORWARD_LAUNCH_SLOTS = 4
PPO_VALUE_GRAD_LAUNCH_SLOTS = 4
# policy evaluation (include/atc_step.h: atc_policy_eval): the words of the per-env record (int32 [B, EVAL_WORDS]; words 7 .. 10 are float32
# bit patterns, words 13 .. 15 reserved), EVAL_CLEAR the flag of atc_policy_eval_out_t that starts the record afresh; its record counts by
# width and K in (0, 1, 2, 4) like the rollout with episode ends
(EVAL_EPISODES, EVAL_WINS, EVAL_END_BELOW_MVA, EVAL_END_OUTSIDE, EVAL_END_CONFLICT, EVAL_END_TIMEOUT, EVAL_STEPS, EVAL_RETURN_SUM, EVAL_RETURN_SQ,
 EVAL_RETURN_MIN, EVAL_RETURN_MAX, EVAL_FLAGS_OR, EVAL_LAUNCH_STEPS) = range(13)
EVAL_WORDS = 16
EVAL_CLEAR = 1
POLICY_EVAL_LAUNCH_SLOTS = 28
# advantage normalisation (include/atc_step.h: atc_adv_normalise): tiles of ADV_TILE rows, at most ADV_MAX_WG workgroups = triples of `scratch`
# (float64 [G, 3]), ADV_DEFAULT_WG where the caller leaves the choice to the library; the words of `stats`; one slot, one count per call
ADV_TILE = 256
ADV_MAX_WG = 1024
ADV_DEFAULT_WG = 256
ADV_STATS = 4
ADV_STAT_N, ADV_STAT_MEAN, ADV_STAT_SCALE, ADV_STAT_STD = range(4)
ADV_NORMALISE_LAUNCH_SLOTS = 1
# the optimiser step (include/atc_step.h: atc_adam_step): one workgroup of ADAM_BLOCK lanes over at most ADAM_MAX_WORDS words per tensor; the
# words of `stats`; its record counts calls by the number of tensors (slot = n_tensors - 1)
ADAM_BLOCK = 1024
ADAM_MAX_WORDS = 65536
ADAM_STATS = 4
ADAM_STAT_NORM, ADAM_STAT_COEF, ADAM_STAT_SKIPPED, ADAM_STAT_STEP = range(4)
ADAM_STEP_LAUNCH_SLOTS = 2
# decisions of the packed policy outside a rollout (include/atc_step.h: atc_policy_forward): at most POLICY_FWD_MAX_SAMPLES draws per row in one
# call; its record counts calls by K in (0, 1, 2, 4)
POLICY_FWD_MAX_SAMPLES = 64
POLICY_FORWARD_LAUNCH_SLOTS = 4
# candidates continued by the policy inside the launch (include/atc_step.h: atc_lookahead_policy): K, H and M are the drawn plans' (SKIP_MAX,
# PLAN_MAX_H, SAMPLE_MAX_M); its own launch record (slot = log2(W))
LOOKAHEAD_POLICY_LAUNCH_SLOTS = 7


def policy_in(traffic=0):
    """width of the policy's input row: POLICY_IN own words + 7 per traffic record (ATC_POLICY_TRAFFIC_IN)"""
    return POLICY_IN + POLICY_TRAFFIC_WORDS_PER_RECORD * int(traffic)


def policy_words(traffic=0):
    """floats in the packed weight array (ATC_POLICY_WORDS; ATC_POLICY_TRAFFIC_WORDS(K))"""
    return POLICY_WORDS + POLICY_HIDDEN * POLICY_TRAFFIC_WORDS_PER_RECORD * int(traffic)


def value_words(traffic=0):
    """floats in the packed critic (ATC_VALUE_WORDS(K))"""
    return VALUE_WORDS + POLICY_HIDDEN * POLICY_TRAFFIC_WORDS_PER_RECORD * int(traffic)


def ppo_grad_workgroups(R, workgroups=0):
    """G of an atc_ppo_policy_grad or atc_ppo_value_grad call on R rows: `workgroups`, or with 0 min(tiles of 64 rows, PPO_GRAD_DEFAULT_WG); `scratch` has G rows"""
    return int(workgroups) if workgroups else min((int(R) + PPO_GRAD_TILE - 1) // PPO_GRAD_TILE, PPO_GRAD_DEFAULT_WG)


def adv_workgroups(R, workgroups=0):
    """G of an atc_adv_normalise call on R rows: `workgroups`, or with 0 min(tiles of 256 rows, ADV_DEFAULT_WG); `scratch` is float64 [G, 3]"""
    return int(workgroups) if workgroups else min((int(R) + ADV_TILE - 1) // ADV_TILE, ADV_DEFAULT_WG)
