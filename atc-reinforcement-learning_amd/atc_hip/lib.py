"""ctypes binding of libatcstep.so (include/atc_step.h).  No CPU fallback: importing works anywhere, but every compute
entry point raises if the library is missing or there is no GPU."""
import ctypes as C
import os

import numpy as np

from . import layout as L

HERE = os.path.dirname(os.path.abspath(__file__))
_lib = None
LIB_PATH = os.path.join(HERE, "libatcstep.so")  # the in-tree build; nothing in the environment can redirect it


def use_library(path):
    """Developer tools that A/B kernel build variants (bench.py --lib, tools/) name the variant explicitly, before the first
    load; the product never calls this."""
    global LIB_PATH
    if _lib is not None:
        raise RuntimeError("libatcstep.so is already loaded")
    LIB_PATH = os.path.abspath(path)


class AtcParams(C.Structure):
    """atc_params_t"""
    _fields_ = [("dt", C.c_double), ("timestep_limit", C.c_int32), ("mode", C.c_uint32), ("seed", C.c_uint64),
                ("sep_nm", C.c_float), ("sep_ft", C.c_float), ("conflict_reward", C.c_float), ("reserved0", C.c_uint32),
                ("reserved1", C.c_float), ("reserved2", C.c_uint32)]


STATE_FIELDS = ("ac", "alt", "last_act", "env", "stats", "phi_wide")
OUT_FIELDS = ("obs", "raw_obs", "reward", "ac_reward", "done", "flags", "min_sep", "term_obs", "packet")


class AtcState(C.Structure):
    """atc_state_t"""
    _fields_ = [(n, C.c_void_p) for n in STATE_FIELDS]


class AtcOut(C.Structure):
    """atc_out_t"""
    _fields_ = [(n, C.c_void_p) for n in OUT_FIELDS]


LOOKAHEAD_FIELDS = ("reward", "done", "n_steps", "flags", "ac_reward", "min_sep", "obs")


class AtcLookaheadOut(C.Structure):
    """atc_lookahead_out_t"""
    _fields_ = [(n, C.c_void_p) for n in LOOKAHEAD_FIELDS]


PLAN_FIELDS = ("reward", "done", "n_steps", "seg_reward", "flags", "ac_reward", "min_sep", "obs")


class AtcPlanOut(C.Structure):
    """atc_plan_out_t"""
    _fields_ = [(n, C.c_void_p) for n in PLAN_FIELDS]


LOOKAHEAD_POLICY_FIELDS = PLAN_FIELDS + ("flown", "logp")


class AtcLookaheadPolicyOut(C.Structure):
    """atc_lookahead_policy_out_t"""
    _fields_ = [(n, C.c_void_p) for n in LOOKAHEAD_POLICY_FIELDS]


PLAN_DRAW_FIELDS = ("seed", "iteration", "flags")


class AtcPlanDraw(C.Structure):
    """atc_plan_draw_t"""
    _fields_ = [("seed", C.c_uint64), ("iteration", C.c_uint32), ("flags", C.c_uint32)]


PLAN_SCORE_FIELDS = ("mode", "elites", "gamma", "temperature")


class AtcPlanScore(C.Structure):
    """atc_plan_score_t"""
    _fields_ = [("mode", C.c_uint32), ("elites", C.c_int32), ("gamma", C.c_float), ("temperature", C.c_float)]


POLICY_FIELDS = ("w", "n_hidden", "flags", "seed", "decision0", "reserved")


class AtcPolicy(C.Structure):
    """atc_policy_t"""
    _fields_ = [("w", C.c_void_p), ("n_hidden", C.c_int32), ("flags", C.c_uint32), ("seed", C.c_uint64), ("decision0", C.c_uint32),
                ("reserved", C.c_uint32)]


POLICY_OUT_FIELDS = ("obs", "reward", "done", "flags", "action", "logp")


class AtcPolicyOut(C.Structure):
    """atc_policy_out_t"""
    _fields_ = [(n, C.c_void_p) for n in POLICY_OUT_FIELDS]


POLICY_TRAFFIC_FIELDS = POLICY_FIELDS + ("traffic_k",)


class AtcPolicyTraffic(C.Structure):
    """atc_policy_traffic_t"""
    _fields_ = AtcPolicy._fields_ + [("traffic_k", C.c_int32)]


POLICY_TRAFFIC_OUT_FIELDS = POLICY_OUT_FIELDS + ("traffic",)


class AtcPolicyTrafficOut(C.Structure):
    """atc_policy_traffic_out_t"""
    _fields_ = [(n, C.c_void_p) for n in POLICY_TRAFFIC_OUT_FIELDS]


POLICY_ENDS_OUT_FIELDS = POLICY_TRAFFIC_OUT_FIELDS + ("term_obs", "term_flags", "control")


class AtcPolicyEndsOut(C.Structure):
    """atc_policy_ends_out_t"""
    _fields_ = [(n, C.c_void_p) for n in POLICY_ENDS_OUT_FIELDS]


POLICY_TERM_OUT_FIELDS = POLICY_ENDS_OUT_FIELDS + ("term_traffic",)


class AtcPolicyTermOut(C.Structure):
    """atc_policy_term_out_t"""
    _fields_ = [(n, C.c_void_p) for n in POLICY_TERM_OUT_FIELDS]


POLICY_EVAL_OUT_FIELDS = ("record", "obs_last", "flags")


class AtcPolicyEvalOut(C.Structure):
    """atc_policy_eval_out_t"""
    _fields_ = [("record", C.c_void_p), ("obs_last", C.c_void_p), ("flags", C.c_uint32)]


GAE_FIELDS = ("gamma", "lam", "flags", "_pad")


class AtcGae(C.Structure):
    """atc_gae_t"""
    _fields_ = [("gamma", C.c_float), ("lam", C.c_float), ("flags", C.c_uint32), ("_pad", C.c_uint32)]


GAE_OUT_FIELDS = ("adv", "ret", "block_reward", "block_done", "block_steps")


class AtcGaeOut(C.Structure):
    """atc_gae_out_t"""
    _fields_ = [(n, C.c_void_p) for n in GAE_OUT_FIELDS]


PPO_GRAD_FIELDS = ("traffic_k", "clip", "adv_shift", "adv_scale", "workgroups", "_pad")


class AtcPpoGrad(C.Structure):
    """atc_ppo_grad_t"""
    _fields_ = [("traffic_k", C.c_int32), ("clip", C.c_float), ("adv_shift", C.c_float), ("adv_scale", C.c_float), ("workgroups", C.c_int32),
                ("_pad", C.c_uint32)]


PPO_GRAD_OUT_FIELDS = ("grad", "stats", "logp_new", "scratch")


class AtcPpoGradOut(C.Structure):
    """atc_ppo_grad_out_t"""
    _fields_ = [(n, C.c_void_p) for n in PPO_GRAD_OUT_FIELDS]


PPO_VALUE_GRAD_FIELDS = ("clip", "workgroups")


class AtcPpoValueGrad(C.Structure):
    """atc_ppo_value_grad_t"""
    _fields_ = [("clip", C.c_float), ("workgroups", C.c_int32)]


PPO_VALUE_GRAD_OUT_FIELDS = ("grad", "stats", "value", "scratch")


class AtcPpoValueGradOut(C.Structure):
    """atc_ppo_value_grad_out_t"""
    _fields_ = [(n, C.c_void_p) for n in PPO_VALUE_GRAD_OUT_FIELDS]


ADV_NORM_FIELDS = ("eps", "workgroups")


class AtcAdvNorm(C.Structure):
    """atc_adv_norm_t"""
    _fields_ = [("eps", C.c_float), ("workgroups", C.c_int32)]


ADV_NORM_OUT_FIELDS = ("out_adv", "stats", "scratch")


class AtcAdvNormOut(C.Structure):
    """atc_adv_norm_out_t"""
    _fields_ = [(n, C.c_void_p) for n in ADV_NORM_OUT_FIELDS]


ADAM_TENSOR_FIELDS = ("w", "grad", "m", "v", "words", "grad_scale", "add_first", "add_count", "add_value")


class AtcAdamTensor(C.Structure):
    """atc_adam_tensor_t"""
    _fields_ = [("w", C.c_void_p), ("grad", C.c_void_p), ("m", C.c_void_p), ("v", C.c_void_p), ("words", C.c_int32), ("grad_scale", C.c_float),
                ("add_first", C.c_int32), ("add_count", C.c_int32), ("add_value", C.c_float)]


ADAM_FIELDS = ("lr", "beta1", "beta2", "eps", "max_norm", "step")


class AtcAdam(C.Structure):
    """atc_adam_t"""
    _fields_ = [("lr", C.c_double), ("beta1", C.c_double), ("beta2", C.c_double), ("eps", C.c_double), ("max_norm", C.c_double), ("step", C.c_int32)]


POLICY_FWD_FIELDS = ("traffic_k", "samples", "rows_per_decision", "flags", "seed", "decision0", "reserved")


class AtcPolicyFwd(C.Structure):
    """atc_policy_fwd_t"""
    _fields_ = [("traffic_k", C.c_int32), ("samples", C.c_int32), ("rows_per_decision", C.c_int32), ("flags", C.c_uint32), ("seed", C.c_uint64),
                ("decision0", C.c_uint32), ("reserved", C.c_uint32)]


POLICY_FWD_OUT_FIELDS = ("mean", "action", "flown", "logp")


class AtcPolicyFwdOut(C.Structure):
    """atc_policy_fwd_out_t"""
    _fields_ = [(n, C.c_void_p) for n in POLICY_FWD_OUT_FIELDS]


class AtcStepCall(C.Structure):
    """atc_step_call_t"""
    _fields_ = [("s", C.c_void_p), ("B", C.c_int32), ("N", C.c_int32), ("st", C.POINTER(AtcState)), ("actions", C.c_void_p),
                ("out", C.POINTER(AtcOut)), ("p", C.POINTER(AtcParams)), ("stream", C.c_void_p)]


EXPORTS = ("atc_abi_version", "atc_last_error", "atc_launch_counts", "atc_host_mapped_ptr", "atc_scenario_create", "atc_scenario_destroy",
           "atc_scenario_attach_lds_table", "atc_query_mva", "atc_query_mva_lds",
           "atc_query_mva_index", "atc_query_corridor", "atc_query_shaping", "atc_reset", "atc_observe", "atc_step",
           "atc_step_multi", "atc_step_packet", "atc_rollout", "atc_rollout_hold", "atc_serve_start", "atc_serve_step", "atc_serve_stop",
           "atc_step_skip", "atc_skip_launch_counts", "atc_fill_prefetch_info", "atc_observe_traffic", "atc_traffic_launch_counts",
           "atc_lookahead", "atc_lookahead_launch_counts", "atc_lookahead_set_mapping", "atc_lookahead_plan", "atc_plan_launch_counts",
           "atc_branch", "atc_branch_launch_counts", "atc_state_select", "atc_select_launch_counts",
           "atc_plan_draw", "atc_lookahead_plan_sampled", "atc_plan_sampled_launch_counts", "atc_plan_draw_launch_counts",
           "atc_plan_refit", "atc_plan_refit_launch_counts", "atc_plan_score", "atc_plan_score_launch_counts",
           "atc_rollout_policy", "atc_rollout_policy_launch_counts", "atc_rollout_policy_traffic", "atc_rollout_policy_traffic_launch_counts",
           "atc_gae", "atc_gae_launch_counts", "atc_rollout_policy_ends", "atc_rollout_policy_ends_launch_counts", "atc_gae_boot",
           "atc_gae_boot_launch_counts", "atc_ppo_policy_grad", "atc_ppo_policy_grad_launch_counts",
           "atc_value_forward", "atc_value_forward_launch_counts", "atc_ppo_value_grad", "atc_ppo_value_grad_launch_counts",
           "atc_policy_eval", "atc_policy_eval_launch_counts", "atc_adv_normalise", "atc_adv_normalise_launch_counts",
           "atc_adam_step", "atc_adam_step_launch_counts", "atc_policy_forward", "atc_policy_forward_launch_counts",
           "atc_lookahead_policy", "atc_lookahead_policy_launch_counts", "atc_rollout_policy_term", "atc_rollout_policy_term_launch_counts")

def load():
    """Loads libatcstep.so; raises (never falls back) when it has not been built."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise RuntimeError("libatcstep.so is missing (%s): build it with `python atc-reinforcement-learning_amd/build.py` "
                           "or __graft_entry__.build(); there is no CPU fallback for the step path" % LIB_PATH)
    import torch  # noqa: F401  — first, so that libatcstep.so binds to the HIP runtime PyTorch-ROCm already loaded
    lib = C.CDLL(LIB_PATH)
    vp, ci = C.c_void_p, C.c_int
    # (the ABI number did not change when atc_step_skip / atc_observe_traffic / atc_lookahead / atc_lookahead_plan were added, so it does not catch a library built before them)
    missing = [name for name in EXPORTS if not hasattr(lib, name)]
    if missing:
        raise RuntimeError("libatcstep.so lacks %s — rebuild" % ", ".join(missing))
    lib.atc_abi_version.restype = ci
    lib.atc_last_error.restype = C.c_char_p
    lib.atc_host_mapped_ptr.argtypes = [vp, C.POINTER(vp)]
    lib.atc_scenario_create.argtypes = [vp, C.c_size_t, ci, C.POINTER(vp)]
    lib.atc_scenario_destroy.argtypes = [vp]
    lib.atc_scenario_attach_lds_table.argtypes = [vp, vp, C.c_size_t]
    lib.atc_query_mva_lds.argtypes = [vp, ci, vp, vp, vp, vp, vp]
    lib.atc_query_mva.argtypes = [vp, ci, vp, vp, vp, ci, vp]
    lib.atc_query_mva_index.argtypes = [vp, ci, vp, vp, vp, ci, vp]
    lib.atc_query_corridor.argtypes = [vp, ci, vp, vp, vp, vp, ci, vp, vp]
    lib.atc_query_shaping.argtypes = [vp, ci, vp, vp, vp, vp, vp, vp, vp]
    lib.atc_reset.argtypes = [vp, ci, ci, C.POINTER(AtcState), vp, vp, C.POINTER(AtcParams), ci, vp]
    lib.atc_observe.argtypes = [vp, ci, ci, C.POINTER(AtcState), vp, vp, C.POINTER(AtcParams), vp]
    lib.atc_step_packet.argtypes = [vp, C.POINTER(AtcState), vp, C.POINTER(AtcOut), C.POINTER(AtcParams), C.c_uint32, vp, vp, ci, vp]
    lib.atc_step.argtypes = [vp, ci, ci, C.POINTER(AtcState), vp, C.POINTER(AtcOut), C.POINTER(AtcParams), vp]
    lib.atc_serve_start.argtypes = [vp, C.POINTER(AtcState), C.POINTER(AtcOut), C.POINTER(AtcParams), vp, C.c_uint32, ci, vp]
    lib.atc_serve_step.argtypes = [vp, vp, C.c_uint32, vp, vp, ci]
    lib.atc_serve_stop.argtypes = [vp, vp]
    lib.atc_step_multi.argtypes = [ci, C.POINTER(AtcStepCall)]
    lib.atc_rollout.argtypes = [vp, ci, ci, ci, C.POINTER(AtcState), vp, C.POINTER(AtcOut), C.POINTER(AtcParams), vp]
    lib.atc_rollout_hold.argtypes = [vp, ci, ci, ci, ci, C.POINTER(AtcState), vp, C.POINTER(AtcOut), C.POINTER(AtcParams), vp]
    lib.atc_step_skip.argtypes = [vp, ci, ci, ci, C.POINTER(AtcState), vp, C.POINTER(AtcOut), vp, C.POINTER(AtcParams), vp]
    lib.atc_fill_prefetch_info.argtypes = [vp, ci, ci, C.POINTER(ci), C.POINTER(ci)]
    lib.atc_observe_traffic.argtypes = [vp, ci, ci, ci, C.POINTER(AtcState), vp, C.POINTER(AtcParams), vp]
    lib.atc_lookahead.argtypes = [vp, ci, ci, ci, ci, C.POINTER(AtcState), vp, C.POINTER(AtcLookaheadOut), C.POINTER(AtcParams), vp]
    lib.atc_lookahead_set_mapping.argtypes = [ci]
    lib.atc_lookahead_plan.argtypes = [vp, ci, ci, ci, ci, ci, C.POINTER(AtcState), vp, C.POINTER(AtcPlanOut), C.POINTER(AtcParams), vp]
    lib.atc_plan_draw.argtypes = [vp, ci, ci, ci, ci, vp, vp, C.POINTER(AtcPlanDraw), vp, ci, vp, C.POINTER(AtcParams), vp]
    lib.atc_lookahead_plan_sampled.argtypes = [vp, ci, ci, ci, ci, ci, C.POINTER(AtcState), vp, vp, C.POINTER(AtcPlanDraw), C.POINTER(AtcPlanOut),
                                               C.POINTER(AtcParams), vp]
    lib.atc_plan_refit.argtypes = [vp, ci, ci, ci, ci, vp, vp, C.POINTER(AtcPlanDraw), vp, vp, vp, C.POINTER(AtcParams), vp]
    lib.atc_plan_score.argtypes = [vp, ci, ci, ci, vp, vp, C.POINTER(AtcPlanScore), vp, vp, vp, ci, vp]
    lib.atc_branch.argtypes = [vp, ci, ci, ci, ci, C.POINTER(AtcState), vp, C.POINTER(AtcState), C.POINTER(AtcLookaheadOut), C.POINTER(AtcParams), vp]
    lib.atc_state_select.argtypes = [vp, ci, ci, C.POINTER(AtcState), ci, C.POINTER(AtcState), vp, vp, vp]
    lib.atc_rollout_policy.argtypes = [vp, ci, ci, ci, ci, C.POINTER(AtcState), vp, C.POINTER(AtcPolicy), C.POINTER(AtcPolicyOut), C.POINTER(AtcParams), vp]
    lib.atc_rollout_policy_traffic.argtypes = [vp, ci, ci, ci, ci, C.POINTER(AtcState), vp, C.POINTER(AtcPolicyTraffic), C.POINTER(AtcPolicyTrafficOut),
                                               C.POINTER(AtcParams), vp]
    lib.atc_gae.argtypes = [vp, ci, ci, ci, ci, vp, vp, vp, vp, C.POINTER(AtcGae), C.POINTER(AtcGaeOut), vp]
    lib.atc_rollout_policy_ends.argtypes = [vp, ci, ci, ci, ci, C.POINTER(AtcState), vp, C.POINTER(AtcPolicyTraffic), C.POINTER(AtcPolicyEndsOut),
                                            C.POINTER(AtcParams), vp]
    lib.atc_rollout_policy_term.argtypes = [vp, ci, ci, ci, ci, C.POINTER(AtcState), vp, C.POINTER(AtcPolicyTraffic), C.POINTER(AtcPolicyTermOut),
                                            C.POINTER(AtcParams), vp]
    lib.atc_policy_eval.argtypes = [vp, ci, ci, ci, ci, C.POINTER(AtcState), vp, C.POINTER(AtcPolicyTraffic), C.POINTER(AtcPolicyEvalOut),
                                    C.POINTER(AtcParams), vp]
    lib.atc_gae_boot.argtypes = [vp, ci, ci, ci, ci, vp, vp, vp, vp, vp, vp, C.POINTER(AtcGae), C.POINTER(AtcGaeOut), vp]
    lib.atc_ppo_policy_grad.argtypes = [vp, ci, ci, vp, vp, vp, vp, vp, vp, vp, vp, C.POINTER(AtcPpoGrad), C.POINTER(AtcPpoGradOut), vp]
    lib.atc_value_forward.argtypes = [vp, ci, ci, vp, vp, vp, vp]
    lib.atc_ppo_value_grad.argtypes = [vp, ci, ci, ci, vp, vp, vp, vp, vp, vp, vp, C.POINTER(AtcPpoValueGrad), C.POINTER(AtcPpoValueGradOut), vp]
    lib.atc_adv_normalise.argtypes = [vp, ci, vp, vp, C.POINTER(AtcAdvNorm), C.POINTER(AtcAdvNormOut), vp]
    lib.atc_adam_step.argtypes = [vp, ci, C.POINTER(AtcAdamTensor), C.POINTER(AtcAdam), vp, vp]
    lib.atc_policy_forward.argtypes = [vp, ci, vp, vp, vp, C.POINTER(AtcPolicyFwd), C.POINTER(AtcPolicyFwdOut), vp]
    lib.atc_lookahead_policy.argtypes = [vp, ci, ci, ci, ci, ci, C.POINTER(AtcState), vp, vp, C.POINTER(AtcPolicy), C.POINTER(AtcLookaheadPolicyOut),
                                         C.POINTER(AtcParams), vp]
    for getter in LAUNCH_RECORDS:
        getattr(lib, getter).argtypes = [C.POINTER(C.c_uint64), ci]
    for name in EXPORTS:
        if name not in ("atc_abi_version", "atc_last_error"):
            getattr(lib, name).restype = ci
    if lib.atc_abi_version() != L.ABI_VERSION:
        raise RuntimeError("libatcstep.so ABI %d != python layout ABI %d — rebuild" % (lib.atc_abi_version(), L.ABI_VERSION))
    _lib = lib
    return lib


def check(rc):
    if rc != 0:
        raise RuntimeError("libatcstep: %s (code %d)" % (load().atc_last_error().decode(), rc))


def launch_name(slot):
    """Readable name of a launch-record slot (include/atc_step.h, ABI 22): "<W>/<form>" for the step kernel's instantiations."""
    if slot == L.LAUNCH_SERVE:
        return "serve"
    return "%d/%s" % (1 << (slot // L.LF_FORMS), L.LF_NAMES[slot % L.LF_FORMS])


def _width(slot):
    return 1 << slot


def _width_k(slot):
    """(W, K) of a slot of the traffic policy rollout's record: slot = 3 log2(W) + log2(K)"""
    return (1 << (slot // 3), 1 << (slot % 3))


def _width_k0(slot):
    """(W, K) of a slot of the record of the policy rollout with episode ends: slot = 4 log2(W) + {0, 1, 2, 3 for K = 0, 1, 2, 4}"""
    return (1 << (slot // 4), (0, 1, 2, 4)[slot % 4])


def _traffic_k0(slot):
    """K of a slot of the PPO policy gradient's record, and of the critic's two: slot = {0, 1, 2, 3 for K = 0, 1, 2, 4}"""
    return (0, 1, 2, 4)[slot]


def _tensors(slot):
    """number of tensors of a slot of the optimiser step's record: slot = n_tensors - 1"""
    return slot + 1


# The library's launch records (include/atc_step.h): getter -> (slots, name of a slot: a function of the slot number, or the one
# slot's name).  load() gives every getter its argtypes from this table; each has a wrapper below, and launch_records() reads all.
LAUNCH_RECORDS = {
    "atc_launch_counts": (L.LAUNCH_SLOTS, launch_name),
    "atc_skip_launch_counts": (L.SKIP_LAUNCH_SLOTS, _width),
    "atc_traffic_launch_counts": (L.TRAFFIC_LAUNCH_SLOTS, _width),
    "atc_lookahead_launch_counts": (L.LOOKAHEAD_LAUNCH_SLOTS, _width),
    "atc_plan_launch_counts": (L.PLAN_LAUNCH_SLOTS, _width),
    "atc_plan_sampled_launch_counts": (L.PLAN_SAMPLED_LAUNCH_SLOTS, _width),
    "atc_plan_draw_launch_counts": (L.PLAN_DRAW_LAUNCH_SLOTS, "draw"),
    "atc_plan_refit_launch_counts": (L.PLAN_REFIT_LAUNCH_SLOTS, "refit"),
    "atc_plan_score_launch_counts": (L.PLAN_SCORE_LAUNCH_SLOTS, "score"),
    "atc_branch_launch_counts": (L.BRANCH_LAUNCH_SLOTS, _width),
    "atc_select_launch_counts": (L.SELECT_LAUNCH_SLOTS, "select"),
    "atc_rollout_policy_launch_counts": (L.ROLLOUT_POLICY_LAUNCH_SLOTS, _width),
    "atc_rollout_policy_traffic_launch_counts": (L.ROLLOUT_POLICY_TRAFFIC_LAUNCH_SLOTS, _width_k),
    "atc_gae_launch_counts": (L.GAE_LAUNCH_SLOTS, "gae"),
    "atc_rollout_policy_ends_launch_counts": (L.ROLLOUT_POLICY_ENDS_LAUNCH_SLOTS, _width_k0),
    "atc_gae_boot_launch_counts": (L.GAE_BOOT_LAUNCH_SLOTS, "gae_boot"),
    "atc_ppo_policy_grad_launch_counts": (L.PPO_GRAD_LAUNCH_SLOTS, _traffic_k0),
    "atc_value_forward_launch_counts": (L.VALUE_FORWARD_LAUNCH_SLOTS, _traffic_k0),
    "atc_ppo_value_grad_launch_counts": (L.PPO_VALUE_GRAD_LAUNCH_SLOTS, _traffic_k0),
    "atc_policy_eval_launch_counts": (L.POLICY_EVAL_LAUNCH_SLOTS, _width_k0),
    "atc_adv_normalise_launch_counts": (L.ADV_NORMALISE_LAUNCH_SLOTS, "adv_normalise"),
    "atc_adam_step_launch_counts": (L.ADAM_STEP_LAUNCH_SLOTS, _tensors),
    "atc_policy_forward_launch_counts": (L.POLICY_FORWARD_LAUNCH_SLOTS, _traffic_k0),
    "atc_lookahead_policy_launch_counts": (L.LOOKAHEAD_POLICY_LAUNCH_SLOTS, _width),
    "atc_rollout_policy_term_launch_counts": (L.ROLLOUT_POLICY_TERM_LAUNCH_SLOTS, _width_k),
}


def _counts(getter):
    """{name of slot: count} of one of the library's launch records (`getter`: a key of LAUNCH_RECORDS), zero counts left out."""
    slots, name = LAUNCH_RECORDS[getter]
    buf = (C.c_uint64 * slots)()
    check(getattr(load(), getter)(buf, slots))
    return {name(i) if callable(name) else name: int(v) for i, v in enumerate(buf) if v}


def launch_records():
    """Every launch record of the calling thread in one dict, keyed by getter name: {"atc_launch_counts": launch_counts(), ...,
    "atc_select_launch_counts": select_launch_counts()}.  Equal before and after a block of code: nothing in it launched."""
    return {getter: _counts(getter) for getter in LAUNCH_RECORDS}


def launch_counts():
    """Launches made by the calling thread so far, per kernel instantiation: {"16/allv-multi": n, ..., "serve": n}, names with a
    count of zero left out.  The counters only grow; take the difference of two calls around a block of code."""
    return _counts("atc_launch_counts")


def skip_launch_counts():
    """Launches of the frame-skip kernel (atc_step_skip) made by the calling thread so far, by lane-group width: {16: n, ...},
    widths with a count of zero left out.  Separate from launch_counts(), which a skip call leaves as it is."""
    return _counts("atc_skip_launch_counts")


def traffic_launch_counts():
    """Launches of the traffic-observation kernel (atc_observe_traffic) made by the calling thread so far, by lane-group width:
    {16: n, ...}, widths with a count of zero left out.  Separate from launch_counts() and skip_launch_counts()."""
    return _counts("atc_traffic_launch_counts")


def lookahead_launch_counts():
    """Launches of the look-ahead kernel (atc_lookahead) made by the calling thread so far, by lane-group width: {16: n, ...},
    widths with a count of zero left out.  Separate from the other launch records, which a look-ahead leaves as they are."""
    return _counts("atc_lookahead_launch_counts")


def plan_launch_counts():
    """Launches of the plan look-ahead kernel (atc_lookahead_plan) made by the calling thread so far, by lane-group width:
    {16: n, ...}, widths with a count of zero left out.  Separate from the other launch records, which a plan call leaves as they are."""
    return _counts("atc_plan_launch_counts")


def plan_sampled_launch_counts():
    """Launches of the drawn-plan kernel (atc_lookahead_plan_sampled) made by the calling thread so far, by lane-group width:
    {16: n, ...}, widths with a count of zero left out.  Separate from the other launch records, which a sampled call leaves as they are."""
    return _counts("atc_plan_sampled_launch_counts")


def plan_draw_launch_counts():
    """Launches of the plan materialiser (atc_plan_draw) made by the calling thread so far: {"draw": n}, or {} before the first."""
    return _counts("atc_plan_draw_launch_counts")


def plan_refit_launch_counts():
    """Launches of the refit on drawn plans (atc_plan_refit) made by the calling thread so far: {"refit": n}, or {} before the first."""
    return _counts("atc_plan_refit_launch_counts")


def plan_score_launch_counts():
    """Launches of the scoring and ranking of drawn plans (atc_plan_score) made by the calling thread so far: {"score": n}, or {} before the first."""
    return _counts("atc_plan_score_launch_counts")


def branch_launch_counts():
    """Launches of the branch kernel (atc_branch) made by the calling thread so far, by lane-group width: {16: n, ...}, widths with a
    count of zero left out.  Separate from the other launch records, which a branch call leaves as they are."""
    return _counts("atc_branch_launch_counts")


def select_launch_counts():
    """Launches of the state gather (atc_state_select) made by the calling thread so far: {"select": n}, or {} before the first."""
    return _counts("atc_select_launch_counts")


def rollout_policy_launch_counts():
    """Launches of the policy rollout (atc_rollout_policy) made by the calling thread so far, by lane-group width: {16: n, ...}, widths
    with a count of zero left out.  Separate from the other launch records, which a policy rollout leaves as they are."""
    return _counts("atc_rollout_policy_launch_counts")


def rollout_policy_traffic_launch_counts():
    """Launches of the policy rollout with traffic (atc_rollout_policy_traffic) made by the calling thread so far, by lane-group width and
    records per aircraft: {(16, 4): n, ...}, zero counts left out.  Separate from the other launch records, rollout_policy's included."""
    return _counts("atc_rollout_policy_traffic_launch_counts")


def gae_launch_counts():
    """Launches of the advantages and returns of a collection (atc_gae) made by the calling thread so far: {"gae": n}, or {} before the first."""
    return _counts("atc_gae_launch_counts")


def rollout_policy_ends_launch_counts():
    """Launches of the policy rollout with episode ends (atc_rollout_policy_ends) made by the calling thread so far, by lane-group width and
    records per aircraft (0: the ten-word policy): {(16, 0): n, ...}, zero counts left out.  Separate from the other launch records."""
    return _counts("atc_rollout_policy_ends_launch_counts")


def rollout_policy_term_launch_counts():
    """Launches of the policy rollout with terminal traffic records (atc_rollout_policy_term) made by the calling thread so far, by lane-group
    width and records per aircraft: {(16, 4): n, ...}, zero counts left out.  Separate from the other launch records, rollout_policy_ends' included."""
    return _counts("atc_rollout_policy_term_launch_counts")


def policy_eval_launch_counts():
    """Launches of the policy evaluation (atc_policy_eval) made by the calling thread so far, by lane-group width and records per aircraft
    (0: the ten-word policy): {(16, 0): n, ...}, zero counts left out.  Separate from the other launch records."""
    return _counts("atc_policy_eval_launch_counts")


def gae_boot_launch_counts():
    """Launches of the advantages with bootstrapped truncations (atc_gae_boot) made by the calling thread so far: {"gae_boot": n}, or {}."""
    return _counts("atc_gae_boot_launch_counts")


def ppo_policy_grad_launch_counts():
    """Calls of the PPO policy loss and gradient (atc_ppo_policy_grad; two launches each) made by the calling thread so far, by records per
    aircraft (0: the ten-word policy): {0: n, 4: n, ...}, zero counts left out.  Separate from the other launch records."""
    return _counts("atc_ppo_policy_grad_launch_counts")


def value_forward_launch_counts():
    """Calls of the critic's forward (atc_value_forward; one launch each) made by the calling thread so far, by records per aircraft (0: the
    ten-word row): {0: n, 4: n, ...}, zero counts left out.  Separate from the other launch records."""
    return _counts("atc_value_forward_launch_counts")


def ppo_value_grad_launch_counts():
    """Calls of the PPO value loss and gradient (atc_ppo_value_grad; two launches each) made by the calling thread so far, by records per
    aircraft, like ppo_policy_grad_launch_counts().  Separate from the other launch records."""
    return _counts("atc_ppo_value_grad_launch_counts")


def adv_normalise_launch_counts():
    """Calls of the advantage normalisation (atc_adv_normalise; two launches each) made by the calling thread so far: {"adv_normalise": n},
    or {} before the first.  Separate from the other launch records."""
    return _counts("atc_adv_normalise_launch_counts")


def adam_step_launch_counts():
    """Calls of the optimiser step (atc_adam_step; one launch each) made by the calling thread so far, by the number of tensors: {1: n, 2: n},
    zero counts left out.  Separate from the other launch records."""
    return _counts("atc_adam_step_launch_counts")


def policy_forward_launch_counts():
    """Calls of the stand-alone policy forward (atc_policy_forward; one launch each) made by the calling thread so far, by records per
    aircraft (0: the ten-word policy): {0: n, 4: n, ...}, zero counts left out.  Separate from the other launch records."""
    return _counts("atc_policy_forward_launch_counts")


def lookahead_policy_launch_counts():
    """Launches of the policy look-ahead kernel (atc_lookahead_policy) made by the calling thread so far, by lane-group width: {16: n, ...},
    widths with a count of zero left out.  Separate from the other launch records, which the call leaves as they are."""
    return _counts("atc_lookahead_policy_launch_counts")


def lookahead_set_mapping(candidates_per_workgroup=0):
    """Developer knob (atc_lookahead_set_mapping): candidates a workgroup of the calling thread's later look-aheads (plans included) evaluates;
    1 = one workgroup per (tile, candidate), M = a loop over all candidates, 0 = the library's choice.  Results do not depend on it."""
    check(load().atc_lookahead_set_mapping(int(candidates_per_workgroup)))


def fill_prefetch_info(scenario, B, N):
    """(resident, stride) of the fast single-step launch's fill-phase prefetch for a batch of B x N on `scenario`'s device
    (include/atc_step.h: atc_fill_prefetch_info): the workgroups the device holds at once, and what an atc_step of that batch
    passes to the kernel (0: prefetch off)."""
    resident, stride = C.c_int(0), C.c_int(0)
    check(load().atc_fill_prefetch_info(scenario.handle, int(B), int(N), C.byref(resident), C.byref(stride)))
    return resident.value, stride.value


def mapped_ptr(tensor):
    """Device address of a pinned (hipHostMalloc) CPU tensor: kernels access it zero-copy over the host link."""
    dev = C.c_void_p()
    check(load().atc_host_mapped_ptr(C.c_void_p(tensor.data_ptr()), C.byref(dev)))
    return dev.value


def _torch_cuda():
    import torch
    if not torch.cuda.is_available():
        raise RuntimeError("no GPU visible: the AtcGym step path runs only on the HIP device (no CPU fallback)")
    return torch


def current_stream_ptr(device):
    torch = _torch_cuda()
    return C.c_void_p(torch.cuda.current_stream(device).cuda_stream)


def make_params(dt=1.0, shaping=True, normalize=True, discrete=False, auto_reset=False, random_entry=False, seed=0,
                timestep_limit=6000, sep_nm=3.0, sep_ft=1000.0, conflict_reward=-200.0, keep_active=False):
    mode = (L.M_REWARD_SHAPING if shaping else 0) | (L.M_NORMALIZE if normalize else 0) | \
           (L.M_DISCRETE if discrete else 0) | (L.M_AUTO_RESET if auto_reset else 0) | \
           (L.M_RANDOM_ENTRY if random_entry else 0) | (L.M_KEEP_ACTIVE if keep_active else 0)
    return AtcParams(float(dt), int(timestep_limit), mode, int(seed) & (2 ** 64 - 1), sep_nm, sep_ft, conflict_reward, 0,
                     0.0, 0)


LDS_TOO_LARGE = "larger than the device's LDS per workgroup"   # atc_scenario_attach_lds_table's one refusal that is not an error


class Scenario:
    """Device-resident sector (opaque atc_scenario_t handle) + batched geometry queries."""

    def __init__(self, compiled, device=0, lds_table=False):
        """lds_table=True also attaches the sector's LDS-resident lookup table (include/atc_step.h, ABI 21) where it has one and
        the device's LDS holds it: multi-step launches of one-aircraft envs then answer the MVA lookup from LDS (same results).
        `has_lds_table` tells whether one is attached."""
        torch = _torch_cuda()
        self.has_lds_table = False
        self.compiled = compiled
        self.device = torch.device("cuda", device if isinstance(device, int) else torch.device(device).index or 0)
        self._lib = load()
        self._h = C.c_void_p()
        blob = np.ascontiguousarray(compiled.blob32)
        with torch.cuda.device(self.device):
            check(self._lib.atc_scenario_create(blob.ctypes.data_as(C.c_void_p), blob.size, self.device.index,
                                                C.byref(self._h)))
        if lds_table:
            self.attach_lds_table()

    def attach_lds_table(self):
        """Builds (once per CompiledSector) and attaches the LDS-resident lookup table.  Where the table does not apply — a sector
        without a lookup grid, with noise-abatement areas or otherwise without a table (CompiledSector.lds_table), or a table larger
        than the device's LDS per workgroup — the sector simply keeps stepping from the grid: returns has_lds_table = False.  Any
        other refusal by atc_scenario_attach_lds_table (a malformed table, a HIP error) raises with atc_last_error(): a table that
        should have been attached is never dropped quietly."""
        torch = _torch_cuda()
        self.has_lds_table = False
        tab = self.compiled.lds_table() if self.compiled.has_grid else None
        if tab is not None:
            t = np.ascontiguousarray(tab)
            with torch.cuda.device(self.device):
                rc = self._lib.atc_scenario_attach_lds_table(self._h, t.ctypes.data_as(C.c_void_p), t.nbytes)
            if rc != 0 and LDS_TOO_LARGE not in self._lib.atc_last_error().decode():
                check(rc)
            self.has_lds_table = rc == 0
        return self.has_lds_table

    def query_mva_lds(self, x, y):
        """Airspace.get_mva_height through the attached LDS table: (heights [ft] or -1, answered-from-the-table flags)."""
        torch = _torch_cuda()
        x, y = self._f32(x), self._f32(y)
        out = torch.empty(x.numel(), dtype=torch.int32, device=self.device)
        src = torch.empty(x.numel(), dtype=torch.uint8, device=self.device)
        with torch.cuda.device(self.device):
            check(self._lib.atc_query_mva_lds(self._h, x.numel(), x.data_ptr(), y.data_ptr(), out.data_ptr(), src.data_ptr(),
                                              current_stream_ptr(self.device)))
        return out.cpu().numpy(), src.cpu().numpy()

    @property
    def handle(self):
        return self._h

    def close(self):
        if self._h:
            self._lib.atc_scenario_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _f32(self, v):
        torch = _torch_cuda()
        return torch.as_tensor(np.ascontiguousarray(np.asarray(v, dtype=np.float32).ravel()), device=self.device)

    def _query_mva(self, fn, x, y, use_grid):
        torch = _torch_cuda()
        x, y = self._f32(x), self._f32(y)
        out = torch.empty(x.numel(), dtype=torch.int32, device=self.device)
        with torch.cuda.device(self.device):
            check(fn(self._h, x.numel(), x.data_ptr(), y.data_ptr(), out.data_ptr(), int(use_grid),
                     current_stream_ptr(self.device)))
        return out.cpu().numpy()

    def query_mva(self, x, y, use_grid=True):
        """Airspace.get_mva_height (model.py:291-292) for arrays of points: height [ft] or -1."""
        return self._query_mva(self._lib.atc_query_mva, x, y, use_grid)

    def query_mva_index(self, x, y, use_grid=True):
        return self._query_mva(self._lib.atc_query_mva_index, x, y, use_grid)

    def query_corridor(self, x, y, h, phi, angle_only=False):
        """Runway.inside_corridor (model.py:248-257) / Corridor._inside_corridor_angle (model.py:212-231)."""
        torch = _torch_cuda()
        x, y, h, phi = (self._f32(v) for v in (x, y, h, phi))
        out = torch.empty(x.numel(), dtype=torch.uint8, device=self.device)
        with torch.cuda.device(self.device):
            check(self._lib.atc_query_corridor(self._h, x.numel(), x.data_ptr(), y.data_ptr(), h.data_ptr(),
                                               phi.data_ptr(), int(angle_only), out.data_ptr(),
                                               current_stream_ptr(self.device)))
        return out.cpu().numpy()

    def query_shaping(self, d_faf, phi_rel_faf, phi_plane, h, on_gp):
        """atc_gym.py:199-260 -> [n,3] (position, angle, glideslope)."""
        torch = _torch_cuda()
        a = [self._f32(v) for v in (d_faf, phi_rel_faf, phi_plane, h, on_gp)]
        out = torch.empty((a[0].numel(), 3), dtype=torch.float32, device=self.device)
        with torch.cuda.device(self.device):
            check(self._lib.atc_query_shaping(self._h, a[0].numel(), *[t.data_ptr() for t in a], out.data_ptr(),
                                              current_stream_ptr(self.device)))
        return out.cpu().numpy()
