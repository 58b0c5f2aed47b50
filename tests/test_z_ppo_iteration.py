"""Whole PPO iterations (atc_hip/ppo.py: collect / collect_bootstrap, policy_grad, value_grad, update) against an independent trainer:
tests/ppo_trainer_ref.py, plain torch on the CPU with autograd, clip_grad_norm_ and torch.optim.Adam, fed the stored arrays of the
collection.  Two chained iterations per case on ONE adam_state: the second collects with the updated weights and goes on counting Adam's steps.

CPU: a stand-in env whose adv_normalise, ppo_policy_grad, ppo_value_grad and adam_step are the numpy restatements with float32 stores (and
whose rollout, value forward and GAE return synthetic stored arrays and the restatements of those calls), so that atc_hip.ppo runs unchanged
without a GPU; agreement with the float64 trainer on K in {0, 2}, with and without control, a per-env [D, B] advantage, ragged minibatches, a
K = 2 policy with a K = 0 critic; eight deliberate faults (FAULTS), each caught by a named case; the refusal of a critic of the wrong size.
GPU: four collections, the ragged one twice (GPU_CASES: per aircraft and per env) on envs of helpers.policy_env; the float64 trainer is fed what the device stored.

THE BARS.  None is fixed: the bar of a quantity is 4 x the deviation of the float32 twin (the same trainer code in torch.float32) from the
float64 trainer on the same collection, per part.  Floors, from the number formats alone: a weight part, (Adam steps so far) x
spacing(float32(max |w|)) — one float32 store rounding per step; a stored float32 array or statistic, spacing(float32(max |value|)) — its
own store; KL and max |dlogp|, spacing(float32(max |logp_old|)) — they are sums of differences of float32 logp words (ppo_grad_ref's
STATS_OF_LOGP).  The bar of a per-minibatch statistic is taken over the E x M minibatches of the iteration: one scalar's twin deviation can be
zero by luck.  n, the number of normalised rows and the cut counts are exact under THE MARGIN CONDITION, which is asserted, not skipped on:
in the float64 trainer every participating row of every minibatch lies >= ppo_grad_ref.RATIO_MARGIN from a policy clip boundary, has
|A| >= ppo_grad_ref.ADV_MARGIN, lies >= ppo_value_ref.CLIP_MARGIN from the value clip boundary, and, outside it, >= ppo_value_ref.TIE_MARGIN
from e^2 = ec^2.  Seeds, lr, clip and vclip are chosen so that it holds.

Measured (deviation / bar, the largest over both iterations; reported, not tuned):
  CPU stand-in: see MEASURED_CPU below.
  MI355X:       see MEASURED_GPU below, next to the seeds and the margins observed there.
DESIGN.md section 3r.1."""
import collections

import numpy as np
import pytest

import gae_boot_ref
import gae_ref
import helpers as H
import policy_ref as P
import ppo_grad_ref as G
import ppo_trainer_ref as TR
import ppo_update_ref as U
import ppo_value_ref as PV
from atc_hip import layout as L

UPDATE = dict(clip=0.2, vclip=0.3, lr=1e-3, ent_coef=0.01, vf_coef=0.5, max_grad_norm=0.5, eps=1e-5)
GAMMA, LAM, EPOCHS = 0.99, 0.95, 2
LOG_STD = (-0.5, -1.0, 0.25)

# largest deviation / bar measured over both iterations, per case: (values / adv / ret / normalised adv, per-minibatch statistics, weights)
MEASURED_CPU = {"k0-control": (0.43, 0.82, 0.38), "k2-plain": (0.35, 0.96, 0.78), "per-env-ragged": (0.46, 0.46, 0.39), "mixed-k": (0.36, 0.44, 0.25)}
# MI355X, per case: the seed; the margins observed with it per iteration (ratio, |A|, value clip; the value tie margin is inf: no row leaves
# the value clip range at vclip = 1.0); the largest deviation / bar over both iterations in MEASURED_CPU's order
MEASURED_GPU = {
    "boot": (1, ((9.5e-3, 8.0e-3, 0.57), (3.1e-3, 2.2e-2, 0.57)), (0.42, 0.66, 0.45)),      # 31 time-limit ends, 1 hard end, 3 uncontrolled rows, 15 cut rows
    "traffic": (1, ((1.9e-4, 0.147, 0.42), (1.5e-2, 0.147, 0.39)), (0.55, 0.48, 0.25)),
    "traffic4": (3, ((2.7e-4, 0.221, 0.60), (1.2e-2, 0.699, 0.78)), (0.34, 0.11, 0.02)),      # seeds 1 and 2: a ratio 5.1e-5 / 4.6e-5 from a boundary
    "ragged": (1, ((9.1e-4, 0.231, 0.26), (5.4e-3, 0.196, 0.35)), (0.35, 0.61, 0.25)),
    "ragged-per-env": (1, ((1.0e-3, 0.232, 0.061), (5.1e-3, 0.202, 0.30)), (0.43, 0.36, 0.25)),
}
# NOT EVERY SEED PASSES.  Of the seeds 1 .. 8 that hold the margin condition on the device, these miss a bar: boot 2 (norm, coef 14.3; vw.W1
# 1.09) and 6 (norm, coef 2.5), both in iteration 2; traffic4 5 (w.b3 1.42; iteration 2: policy_loss, kl, max |dlogp| 1.78, w.W1 1.33) and 7
# (w.b1 1.02); ragged 8 (max |dlogp| 1.16).  On the CPU, k0-control with an earlier synthetic draw missed w.b1 at 1.10: one bias word whose
# clipped gradient, 3.3e-6, lies under Adam's eps, where lr eps / (|g| + eps)^2 = 56 multiplies a float32 gradient error of 2.3e-9 (the twin's,
# on that word: 3.3e-10).  4 x ONE twin's deviation is a bar that a correct float32 evaluation exceeds now and then; the seeds are fixed by
# the margin rule alone, not by these figures.


def _np(t):
    return t.detach().cpu().numpy()


# ------------------------------------------------------------------------------------------------------------ the comparison
ARRAYS = ("values", "adv", "ret", "adv_norm")
SCALARS = ("policy_loss", "value_loss", "kl", "ratio", "dlogp_max", "norm", "coef")
OF_LOGP = ("kl", "dlogp_max")
EXACT = ("n", "cut", "vcut")


def _spacing(x):
    return float(np.spacing(np.float32(abs(x))))


def compare(got, r64, r32, stored, K, KV):
    """[(group, name, deviation, bar)] of one iteration; exact quantities have bar 0"""
    rows = []
    ctrl = np.ones(np.asarray(stored["action"]).shape[:3], bool) if stored.get("control") is None else np.asarray(stored["control"]) != 0
    for name in ARRAYS:
        a, b, c = (np.asarray(x[name], np.float64) for x in (got, r64, r32))
        assert a.shape == b.shape, (name, a.shape, b.shape)
        if name == "adv_norm":
            a, b, c = a[ctrl], b[ctrl], c[ctrl]
        rows.append(("arrays", name, float(np.max(np.abs(a - b))), max(4.0 * float(np.max(np.abs(c - b))), _spacing(np.max(np.abs(b))))))
    top_logp = float(np.max(np.abs(np.asarray(stored["logp"], np.float64)[ctrl])))
    for name in SCALARS:
        a, b, c = (np.asarray(x[name], np.float64) for x in (got, r64, r32))
        floor = _spacing(top_logp) if name in OF_LOGP else _spacing(np.max(np.abs(b)))
        rows.append(("stats", name, float(np.max(np.abs(a - b))), max(4.0 * float(np.max(np.abs(c - b))), floor)))
    for name in EXACT + ("adv_n",):
        rows.append(("exact", name, float(np.max(np.abs(np.asarray(got[name], np.float64) - np.asarray(r64[name], np.float64)))), 0.0))
    for key, split, k in (("w", P.split, K), ("vw", PV.split, KV)):
        a, b, c = (split(np.asarray(x[key], np.float64), k) for x in (got, r64, r32))
        for part in b:
            floor = r64["steps"] * _spacing(np.max(np.abs(b[part])))
            rows.append(("weights", "%s.%s" % (key, part), float(np.max(np.abs(a[part] - b[part]))), max(4.0 * float(np.max(np.abs(c[part] - b[part]))), floor)))
    return rows


def report(label, rows):
    """prints deviation / bar of every quantity, returns ({group: largest ratio}, [names that miss])"""
    worst, missed = collections.defaultdict(float), []
    for group, name, dev, bar in rows:
        ratio = dev / bar if bar > 0 else (0.0 if dev == 0 else float("inf"))
        print("%s: %-12s deviation %.3e, bar %.3e, deviation / bar %.3f" % (label, name, dev, bar, ratio))
        worst[group] = max(worst[group], ratio)
        if not dev <= bar:
            missed.append(name)
    print("%s: largest deviation / bar %s" % (label, ", ".join("%s %.3f" % kv for kv in sorted(worst.items()))))
    return dict(worst), missed


def margins_hold(label, m):
    print("%s: margins ratio %.3e, |A| %.3e, value clip %.3e, value tie %.3e" % (label, m["ratio"], m["adv"], m["vclip"], m["vtie"]))
    return m["ratio"] >= G.RATIO_MARGIN and m["adv"] >= G.ADV_MARGIN and m["vclip"] >= PV.CLIP_MARGIN and m["vtie"] >= PV.TIE_MARGIN


def device_result(res, upd, state, w, vw):
    """what an iteration of atc_hip.ppo left, in the trainer's names"""
    D, B, N = res["action"].shape[:3]
    ps, vs, ad = _np(upd["policy_stats"]).astype(np.float64), _np(upd["value_stats"]).astype(np.float64), _np(upd["adam_stats"]).astype(np.float64)
    assert np.array_equal(ps[..., L.PPO_STAT_N], vs[..., 0]) and not ad[..., L.ADAM_STAT_SKIPPED].any()
    return {"values": _np(res["values"]), "adv": _np(res["adv"]), "ret": _np(res["ret"]), "adv_norm": _np(state["adv"][(D, B, N)]["adv"]),
            "adv_n": float(_np(upd["adv_stats"])[L.ADV_STAT_N]), "n": ps[..., L.PPO_STAT_N], "policy_loss": ps[..., L.PPO_STAT_LOSS], "kl": ps[..., L.PPO_STAT_KL],
            "cut": np.rint(ps[..., L.PPO_STAT_CUT] * ps[..., L.PPO_STAT_N]), "ratio": ps[..., L.PPO_STAT_RATIO], "dlogp_max": ps[..., L.PPO_STAT_DLOGP_MAX],
            "value_loss": vs[..., 1], "vcut": np.rint(vs[..., 2] * vs[..., 0]), "norm": ad[..., L.ADAM_STAT_NORM], "coef": ad[..., L.ADAM_STAT_COEF],
            "step": ad[..., L.ADAM_STAT_STEP], "w": _np(w), "vw": _np(vw)}


# ------------------------------------------------------------------------------------------------------------ CPU: the stand-in env
class StandIn:
    """What atc_hip.ppo calls on an env, on the CPU: the update's four calls are the numpy restatements with float32 stores, taking the same
    arguments and out= dicts; the rollout returns the synthetic arrays given to load(); the value forward and GAE are their restatements."""
    device = "cpu"

    def __init__(self, B, N, traffic=0):
        import torch
        self.torch, self.B, self.N, self.traffic_k = torch, B, N, traffic
        self.calls = collections.Counter()
        self.stored = self.obs = None

    def load(self, stored):
        self.stored = stored
        self.obs = self.torch.tensor(stored["obs0"]).reshape(self.B, self.N * 10)

    def _rollout(self, keys):
        self.calls["rollout"] += 1
        return {k: self.torch.tensor(self.stored[k]) for k in ("obs", "reward", "done", "action", "logp") + keys}

    def rollout_policy(self, weights, T, hold=1, seed=0, decision0=0, obs0=None):
        return self._rollout(())

    def rollout_policy_traffic(self, weights, T, traffic, hold=1, seed=0, decision0=0, obs0=None):
        return self._rollout(("traffic",))

    def rollout_policy_ends(self, weights, T, traffic=0, hold=1, seed=0, decision0=0, obs0=None):
        return self._rollout(("term_obs", "term_flags", "control"))

    def observe_traffic(self):
        return self.torch.tensor(self.stored["traffic_final"])

    def value_forward(self, weights, rows):
        self.calls["value_forward"] += 1
        K = (int(rows.shape[-1]) - 10) // 7
        return self.torch.tensor(PV.forward(weights.numpy(), rows.numpy(), K, np.float32).reshape(tuple(rows.shape[:-1])))

    def gae(self, reward, done, values, hold=1, gamma=0.99, lam=0.95, *, per_decision=False):
        self.calls["gae"] += 1
        r = gae_ref.gae(reward.numpy(), done.numpy(), values.numpy(), hold=hold, gamma=gamma, lam=lam, per_decision=per_decision)
        return {k: self.torch.tensor(np.asarray(v)) for k, v in r.items()}

    def gae_boot(self, reward, done, values, boot, trunc, hold=1, gamma=0.99, lam=0.95, *, per_decision=False):
        self.calls["gae"] += 1
        r = gae_boot_ref.gae_boot(reward.numpy(), done.numpy(), values.numpy(), boot.numpy(), trunc.numpy(), hold=hold, gamma=gamma, lam=lam,
                                  per_decision=per_decision)
        return {k: self.torch.tensor(np.asarray(v)) for k, v in r.items()}

    def adv_normalise(self, adv, mask=None, *, eps=1e-8, workgroups=0, out=None):
        self.calls["adv_normalise"] += 1
        r = U.adv_normalise(adv.numpy(), None if mask is None else mask.numpy(), eps, workgroups)
        out["adv"].copy_(self.torch.tensor(r["adv"]))
        out["stats"].copy_(self.torch.tensor(r["stats"]))
        return {"adv": out["adv"], "stats": out["stats"]}

    @staticmethod
    def _case(weights, obs_rows, traffic, mask, index, clip, **more):
        K = 0 if traffic is None else int(traffic.shape[-2])
        return dict(K=K, w=weights.numpy(), obs_rows=obs_rows.numpy(), traffic=None if traffic is None else traffic.numpy(), clip=clip,
                    mask=None if mask is None else mask.numpy(), index=None if index is None else index.numpy(), **{k: v.numpy() for k, v in more.items()})

    def ppo_policy_grad(self, weights, obs_rows, action, logp_old, adv, *, traffic=None, mask=None, index=None, clip=0.2, adv_shift=0.0, adv_scale=1.0,
                        workgroups=0, out=None):
        self.calls["ppo_policy_grad"] += 1
        case = self._case(weights, obs_rows, traffic, mask, index, clip, action=action, logp_old=logp_old, adv=adv)
        assert case["w"].size == P.words(case["K"]), "weights are not packed for the K of the records"
        r = G.evaluate(dict(case, adv_shift=adv_shift, adv_scale=adv_scale), np.float32)
        out["grad"].copy_(self.torch.tensor(r["grad"]))
        out["stats"].copy_(self.torch.tensor(r["stats"]))
        out["logp"][self.torch.tensor(r["part"])] = self.torch.tensor(r["logp"][r["part"]])
        return out

    def ppo_value_grad(self, weights, obs_rows, v_old, ret, *, traffic=None, mask=None, index=None, clip=0.2, workgroups=0, out=None):
        self.calls["ppo_value_grad"] += 1
        case = self._case(weights, obs_rows, traffic, mask, index, clip, v_old=v_old, ret=ret)
        if case["w"].size != PV.words(case["K"]):
            raise ValueError("weights must be the contiguous float32 tensor of %d words" % PV.words(case["K"]))
        r = PV.evaluate(case, np.float32)
        out["grad"].copy_(self.torch.tensor(r["grad"]))
        out["stats"].copy_(self.torch.tensor(r["stats"]))
        out["value"][self.torch.tensor(r["part"])] = self.torch.tensor(r["value"][r["part"]])
        return out

    def adam_step(self, tensors, *, lr, step, beta1=0.9, beta2=0.999, eps=1e-5, max_norm=0.0, out=None):
        self.calls["adam_step"] += 1
        host = [dict({k: t[k].numpy() for k in ("w", "grad", "m", "v")}, **{k: t[k] for k in ("grad_scale", "add") if k in t}) for t in tensors]
        new, stats = U.adam_step(host, lr=lr, step=step, beta1=beta1, beta2=beta2, eps=eps, max_norm=max_norm)
        for t, n in zip(tensors, new):
            for k in ("w", "m", "v"):
                t[k].copy_(self.torch.tensor(n[k]))
        out.copy_(self.torch.tensor(stats))
        return out


def synthetic(seed, w, B, N, T, hold, K, ends):
    """the stored arrays of a collection that no env flew: random observations, records, rewards and dones; action and logp drawn from the
    packed policy `w` on the rows the decisions see (policy_ref); with `ends` term_obs, term_flags and control"""
    rng = np.random.default_rng([71, seed])
    D = T // hold
    u = lambda *shape: rng.uniform(-1.0, 1.0, shape).astype(np.float32)      # noqa: E731
    s = {"obs0": u(B, N, 10), "obs": u(T, B, N * 10), "reward": rng.normal(0.0, 0.5, (T, B)).astype(np.float32), "done": (rng.random((T, B)) < 0.2).astype(np.uint8)}
    own = np.stack([s["obs0"]] + [s["obs"][d * hold - 1].reshape(B, N, 10) for d in range(1, D)])
    x = own
    if K:
        s["traffic"], s["traffic_final"] = u(D, B, N, K, 8), u(B, N, K, 8)
        x = np.concatenate([own, s["traffic"][..., :7].reshape(D, B, N, 7 * K)], axis=-1)
    mu = P.mlp(w, x, K, np.float64)
    log_std = P.split(w, K)["log_std"].astype(np.float64)
    s["action"] = (mu + np.exp(log_std) * rng.normal(0.0, 1.0, (D, B, N, 3))).astype(np.float32)
    s["logp"] = P.logp64((s["action"].astype(np.float64) - mu) / np.exp(log_std), log_std).astype(np.float32)
    if ends:
        ended = s["done"].reshape(D, hold, B).any(axis=1)
        causes = np.array([L.F_TIMEOUT, L.F_TIMEOUT | L.F_OUTSIDE, L.F_TIMEOUT | L.F_WON, L.F_BELOW_MVA, L.F_CONFLICT | L.F_TIMEOUT, L.F_OUTSIDE])
        cause = causes[(np.cumsum(ended.reshape(-1)) - 1).reshape(D, B) % len(causes)]      # in turn: time-limit ends and hard ends both occur
        s["term_flags"] = np.where(ended, L.TERM_ENDED | cause, 0).astype(np.uint16).view(np.int16)
        s["term_obs"] = np.where(ended[:, :, None, None], u(D, B, N, 10), np.float32(0))
        s["control"] = (rng.random((D, B, N)) < 0.8).astype(np.uint8)
    return s


CPU_CASES = {
    # name: B, N, T, hold, K (policy), KV (critic), ends (collect_bootstrap, control), per_decision, per_env, M
    "k0-control": dict(B=4, N=3, T=12, hold=2, K=0, KV=0, ends=True, per_decision=False, per_env=False, M=2),
    "k2-plain": dict(B=3, N=4, T=5, hold=1, K=2, KV=2, ends=False, per_decision=False, per_env=False, M=2),
    "per-env-ragged": dict(B=5, N=3, T=15, hold=3, K=0, KV=0, ends=False, per_decision=True, per_env=True, M=4),      # R = 75: slices of 18, 19, 19, 19
    "mixed-k": dict(B=3, N=4, T=6, hold=1, K=2, KV=0, ends=False, per_decision=False, per_env=False, M=3),
}
# the smallest seed from 1 at which the margin condition holds in both iterations (per-env-ragged: seed 1 has a ratio 7.2e-5 from a boundary)
CPU_SEEDS = {"k0-control": 1, "k2-plain": 1, "per-env-ragged": 2, "mixed-k": 1}


def _weights(seed, K, KV):
    return (P.random_weights(np.random.default_rng([72, seed, 0]), 1.0, LOG_STD, False, K), PV.random_weights(np.random.default_rng([72, seed, 1]), 1.0, KV))


def _value_fn(env, vw, c):
    def value_fn(rows):
        v = env.value_forward(vw, rows[..., :10 + 7 * c["KV"]].contiguous())
        return v.mean(dim=-1) if c["per_env"] else v
    return value_fn


def _collect(ppo, env, w, vw, c, T, **kw):
    fn = ppo.collect_bootstrap if c["ends"] else ppo.collect
    return fn(env, w, _value_fn(env, vw, c), T, hold=c["hold"], traffic=0 if c["ends"] else c["K"], gamma=GAMMA, lam=LAM, per_decision=c["per_decision"], **kw)


def _inject_env(m, env, fault, steps_per_update):
    """faults c, d, e, f, h: the stand-in's own calls, wrapped"""
    real_adam, real_norm = env.adam_step, env.adv_normalise
    if fault == "c":      # vf_coef ignored
        m.setattr(env, "adam_step", lambda tensors, **kw: real_adam([{k: v for k, v in t.items() if k != "grad_scale"} for t in tensors], **kw))
    if fault == "d":      # the norm clipped per tensor
        def per_tensor(tensors, out=None, **kw):
            real_adam(tensors[1:], out=out.clone(), **kw)
            return real_adam(tensors[:1], out=out, **kw)
        m.setattr(env, "adam_step", per_tensor)
    if fault == "e":      # advantages normalised over all rows although control is given
        m.setattr(env, "adv_normalise", lambda adv, mask=None, **kw: real_norm(adv, None, **kw))
    if fault == "f":      # the count restarted by the second update()
        m.setattr(env, "adam_step", lambda tensors, step, **kw: real_adam(tensors, step=(step - 1) % steps_per_update + 1, **kw))
    if fault == "h":      # the sign of ent_coef
        flip = lambda t: dict(t, add=(t["add"][0], t["add"][1], -t["add"][2])) if "add" in t else t      # noqa: E731
        m.setattr(env, "adam_step", lambda tensors, **kw: real_adam([flip(t) for t in tensors], **kw))


def run_cpu(name, monkeypatch, fault=None, seed=None):
    """two chained iterations of atc_hip.ppo on the stand-in against the trainer: [(iteration, worst, missed, margins hold)]"""
    import torch
    from atc_hip import ppo
    c = CPU_CASES[name]
    seed = CPU_SEEDS[name] if seed is None else seed
    B, N, T, hold, K, KV, M = (c[k] for k in ("B", "N", "T", "hold", "K", "KV", "M"))
    D = T // hold
    R = D * B * N
    w0, vw0 = _weights(seed, K, KV)
    env = StandIn(B, N, K)
    w, vw = torch.tensor(w0), torch.tensor(vw0)
    state = ppo.adam_state(env, w, vw)
    hyper = dict(UPDATE, gamma=GAMMA, lam=LAM)
    r64, r32 = TR.Trainer(w0, vw0, K, torch.float64, KV, **hyper), TR.Trainer(w0, vw0, K, torch.float32, KV, **hyper)
    out = []
    with monkeypatch.context() as m:
        _inject_env(m, env, fault, EPOCHS * M)
        for it in range(2):
            stored = synthetic(seed * 10 + it, w.numpy(), B, N, T, hold, K, c["ends"])
            env.load(stored)
            with monkeypatch.context() as mc:
                if fault == "g":      # a time-limit end not bootstrapped
                    mc.setattr(ppo, "truncated", lambda flags: torch.zeros(tuple(flags.shape), dtype=torch.uint8))
                res = _collect(ppo, env, w, vw, c, T)
            perm = np.stack([np.random.default_rng([73, seed, it, e]).permutation(R) for e in range(EPOCHS)]).astype(np.int32)
            with monkeypatch.context() as mu:
                if fault == "a":      # rows taken from value_rows[1:]
                    real_rows = ppo.value_rows
                    mu.setattr(ppo, "value_rows", lambda *a, **kw: (lambda r: torch.cat([r[1:], r[-1:]]))(real_rows(*a, **kw)))
                if fault == "b":      # the entropy window at the K = 0 offset
                    real_offsets = ppo._policy.offsets
                    mu.setattr(ppo._policy, "offsets", lambda traffic=0: real_offsets(0))
                upd = ppo.update(env, res, w, vw, state, epochs=EPOCHS, minibatches=M, perm=torch.tensor(perm), **UPDATE)
            assert state["t"] == (it + 1) * EPOCHS * M
            got = device_result(res, upd, state, w, vw)
            kw = dict(hold=hold, minibatches=M, per_decision=c["per_decision"], bootstrap=c["ends"], per_env=c["per_env"])
            a, b = r64.iterate(stored, perm, **kw), r32.iterate(stored, perm, **kw)
            label = "%s%s iteration %d" % (name, " fault " + fault if fault else "", it + 1)
            worst, missed = report(label, compare(got, a, b, stored, K, KV))
            out.append((it, worst, missed, margins_hold(label, a["margins"]), a))
    return out


@pytest.mark.parametrize("name", list(CPU_CASES))
def test_update_on_the_stand_in_agrees_with_the_float64_trainer(name, monkeypatch):
    runs = run_cpu(name, monkeypatch)
    for it, worst, missed, held, ref in runs:
        assert held, "the margin condition does not hold in iteration %d: another seed" % (it + 1)
        assert not missed, (it, missed)
    ref = runs[1][4]
    assert ref["steps"] == 2 * EPOCHS * CPU_CASES[name]["M"]
    if name == "k0-control":      # the clip path is exercised, uncontrolled rows occur (time-limit and hard ends: by construction, see synthetic)
        assert sum(r[4]["cut"].sum() for r in runs) > 0 and all(r[4]["adv_n"] < r[4]["adv_norm"].size for r in runs)
    if name == "per-env-ragged":
        assert ref["adv"].ndim == 2 and len({int(n) for n in ref["n"].reshape(-1)}) > 1


# fault: (the case that catches it, the iteration it shows in, quantities of which at least one must miss its bar)
FAULTS = {
    "a": ("k0-control", 0, ("kl", "w.W1", "policy_loss")),
    "b": ("k2-plain", 0, ("w.log_std",)),
    "c": ("k0-control", 0, ("norm",)),
    "d": ("k0-control", 0, ("norm", "coef")),
    "e": ("k0-control", 0, ("adv_n", "adv_norm")),
    "f": ("k2-plain", 1, ("w.W2", "vw.W2")),
    "g": ("k0-control", 0, ("adv", "ret")),
    "h": ("k0-control", 0, ("w.log_std",)),
}


@pytest.mark.parametrize("fault", list(FAULTS))
def test_each_deliberate_fault_is_caught(fault, monkeypatch):
    name, first, names = FAULTS[fault]
    runs = run_cpu(name, monkeypatch, fault)
    missed = runs[first][2]
    print("fault %s on %s: iteration %d misses %s" % (fault, name, first + 1, missed))
    assert set(names) & set(missed), (fault, names, missed)
    if fault == "f":      # the first update is untouched
        assert not runs[0][2]
    if fault == "g":      # ... on the GAE part: the values themselves agree
        assert "values" not in missed


def test_a_critic_of_another_size_is_refused_before_any_call(monkeypatch):
    import torch
    from atc_hip import ppo
    c = CPU_CASES["k2-plain"]
    B, N, T, K = c["B"], c["N"], c["T"], c["K"]
    w0, vw0 = _weights(3, K, K)
    env = StandIn(B, N, K)
    env.load(synthetic(5, w0, B, N, T, 1, K, False))
    w, vw = torch.tensor(w0), torch.tensor(vw0)
    res = _collect(ppo, env, w, vw, c, T)
    perm = torch.stack([torch.randperm(T * B * N) for _ in range(EPOCHS)]).to(torch.int32)
    for bad_k, text in ((1, "the critic must be packed for the collection's K = 2"), (4, "the critic must be packed for the collection's K = 2")):
        bad = torch.tensor(PV.random_weights(np.random.default_rng(1), 1.0, bad_k))
        state = ppo.adam_state(env, w, bad)
        before = dict(env.calls)
        with pytest.raises(ValueError, match=text):
            ppo.update(env, res, w, bad, state, epochs=EPOCHS, minibatches=2, perm=perm, **UPDATE)
        with pytest.raises(ValueError, match=text):
            ppo.value_grad(env, res, bad)
        assert dict(env.calls) == before and state["t"] == 0
    # a K = 0 policy on a collection that stored records: the policy's size is named, not the critic's
    w00, vw00 = _weights(3, 0, 0)
    state = ppo.adam_state(env, torch.tensor(w00), torch.tensor(vw00))
    before = dict(env.calls)
    with pytest.raises(ValueError, match="the policy must be packed for the collection's K = 2"):
        ppo.update(env, res, torch.tensor(w00), torch.tensor(vw00), state, epochs=EPOCHS, minibatches=2, perm=perm, **UPDATE)
    assert dict(env.calls) == before
    assert "collection's" in ppo.update.__doc__ and "K = 0" in ppo.update.__doc__


# ------------------------------------------------------------------------------------------------------------ GPU
CFG = dict(normalize=True, shaping=True, auto_reset=True, timestep_limit=7, spawn="lattice")
GPU_CASES = {
    # name: B, N, T, hold, K, M, the collection, per_decision, per_env (the critic stand-in returns [D + 1, B])
    "boot": dict(B=8, N=4, T=16, hold=2, K=0, KV=0, M=2, ends=True, per_decision=False, per_env=False),
    "traffic": dict(B=8, N=4, T=8, hold=1, K=2, KV=2, M=2, ends=False, per_decision=False, per_env=False),
    "traffic4": dict(B=4, N=8, T=6, hold=1, K=4, KV=4, M=2, ends=False, per_decision=False, per_env=False),
    "ragged": dict(B=5, N=3, T=21, hold=3, K=0, KV=0, M=3, ends=False, per_decision=True, per_env=False),      # R = 105: minibatches of 35 rows
    "ragged-per-env": dict(B=5, N=3, T=21, hold=3, K=0, KV=0, M=3, ends=False, per_decision=True, per_env=True),
}
# vclip on the device: the smallest of 0.3, 0.5, 1.0 at which every case has a seed among 1 .. 8 that holds the margin condition.  The env's
# returns are of the order of 100 against values of the order of 1, so a row just outside the value clip range has e^2 and ec^2 within
# 2 |v - vc| / |ret| of each other: at 0.3 and 0.5 no seed of any case kept ppo_value_ref.TIE_MARGIN in both iterations.  At 1.0 no row
# leaves the range on the device (vcut = 0 in every case); the value clip's cut path is the CPU cases' (k2-plain, per-env-ragged, mixed-k).
GPU_UPDATE = dict(UPDATE, vclip=1.0)
# the smallest seed from 1, chosen on the MI355X, so that the margin condition holds (the collection depends on the device's logf / cosf)
GPU_SEEDS = {"boot": 1, "traffic": 1, "traffic4": 3, "ragged": 1, "ragged-per-env": 1}


def _records():
    from atc_hip import lib
    return lib.launch_records()


def _moved(before, after):
    out = {}
    for getter in after:
        d = {k: v - before[getter].get(k, 0) for k, v in after[getter].items() if v != before[getter].get(k, 0)}
        if d:
            out[getter] = d
    return out


def run_gpu(name, seed=None):
    """two chained iterations on the device against the trainer fed what the device stored: [(iteration, worst, missed, margins hold, ref, stored)]"""
    import torch
    from atc_hip import ppo
    c = GPU_CASES[name]
    seed = GPU_SEEDS[name] if seed is None else seed
    B, N, T, hold, K, KV, M = (c[k] for k in ("B", "N", "T", "hold", "K", "KV", "M"))
    D = T // hold
    R = D * B * N
    env = H.policy_env(CFG, B, N, traffic=K)      # a fresh env per run: the collection is a function of the seed alone
    if name == "boot":      # one aircraft below every MVA: a hard end at the first step; one on the winning state: handed over, out of control
        x, y, _, phi, v = H.FAR_A
        env.set_state(1, 0, x + 10.0, y, 1000.0, phi, v)
        env.set_state(2, 0, *H.WIN_STATE)
        env.observe()
        env.synchronize()
    w0, vw0 = _weights(seed, K, KV)
    dev = lambda a: torch.as_tensor(np.ascontiguousarray(a), device=env.device)      # noqa: E731
    w, vw = dev(w0), dev(vw0)
    state = ppo.adam_state(env, w, vw)
    hyper = dict(GPU_UPDATE, gamma=GAMMA, lam=LAM)
    r64, r32 = TR.Trainer(w0, vw0, K, torch.float64, KV, **hyper), TR.Trainer(w0, vw0, K, torch.float32, KV, **hyper)
    rollout = "atc_rollout_policy_ends_launch_counts" if c["ends"] else "atc_rollout_policy_traffic_launch_counts" if K else "atc_rollout_policy_launch_counts"
    out = []
    for it in range(2):
        before = _records()
        res = _collect(ppo, env, w, vw, c, T, seed=seed, decision0=it * D)
        env.synchronize()
        moved = _moved(before, _records())
        want = {rollout: 1, "atc_value_forward_launch_counts": 1, "atc_gae_boot_launch_counts" if c["ends"] else "atc_gae_launch_counts": 1}
        if K:
            want["atc_traffic_launch_counts"] = 1
        assert {g: sum(d.values()) for g, d in moved.items()} == want and moved["atc_value_forward_launch_counts"] == {KV: 1}, moved
        stored = {k: _np(res[k]) for k in ("obs", "reward", "done", "action", "logp") + (("term_obs", "term_flags", "control") if c["ends"] else ()) + (("traffic",) if K else ())}
        stored["obs0"] = _np(env._collected_obs0[1])
        if K:
            stored["traffic_final"] = _np(env.observe_traffic())      # (the state the rollout left: what collect() itself read)
        gen = torch.Generator().manual_seed(1000 * seed + it)
        perm = torch.stack([torch.randperm(R, generator=gen) for _ in range(EPOCHS)]).to(torch.int32)
        if it == 0 and name == "boot":      # a zero advantage switches the surrogate off: log_std then moves where ent_coef sends it, up
            w2, vw2 = w.clone(), vw.clone()
            ppo.update(env, dict(res, adv=torch.zeros_like(res["adv"])), w2, vw2, ppo.adam_state(env, w2, vw2), epochs=1, minibatches=1, perm=perm.to(env.device), **GPU_UPDATE)
            env.synchronize()
            up = _np(w2)[-3:] - w0[-3:]
            print("boot: log_std under a zero advantage moved by %s" % up)
            assert np.all(up > 0) and np.array_equal(_np(w2)[:-3], w0[:-3])
        before = _records()
        upd = ppo.update(env, res, w, vw, state, epochs=EPOCHS, minibatches=M, perm=perm.to(env.device), **GPU_UPDATE)
        env.synchronize()
        moved = _moved(before, _records())
        assert moved == {"atc_adv_normalise_launch_counts": {"adv_normalise": 1}, "atc_ppo_policy_grad_launch_counts": {K: EPOCHS * M},
                         "atc_ppo_value_grad_launch_counts": {KV: EPOCHS * M}, "atc_adam_step_launch_counts": {2: EPOCHS * M}}, moved
        assert state["t"] == (it + 1) * EPOCHS * M
        got = device_result(res, upd, state, w, vw)
        assert got["step"].reshape(-1).tolist() == list(range(it * EPOCHS * M + 1, (it + 1) * EPOCHS * M + 1))
        kw = dict(hold=hold, minibatches=M, per_decision=c["per_decision"], bootstrap=c["ends"], per_env=c["per_env"])
        a, b = r64.iterate(stored, _np(perm), **kw), r32.iterate(stored, _np(perm), **kw)
        label = "%s seed %d iteration %d" % (name, seed, it + 1)
        worst, missed = report(label, compare(got, a, b, stored, K, KV))
        out.append((it, worst, missed, margins_hold(label, a["margins"]), a, stored))
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(GPU_CASES))
def test_two_iterations_on_the_device_agree_with_the_float64_trainer(name):
    runs = run_gpu(name)
    c = GPU_CASES[name]
    for it, worst, missed, held, ref, stored in runs:
        assert held, "the margin condition does not hold in iteration %d: another seed" % (it + 1)
        assert not missed, (it, missed)
        assert np.all(ref["n"] > 0) and (c["per_env"]) == (ref["adv"].ndim == 2)
    if name == "boot":
        flags = np.concatenate([r[5]["term_flags"].reshape(-1) for r in runs]).astype(np.int64)
        hard = (flags & (L.F_BELOW_MVA | L.F_OUTSIDE | L.F_CONFLICT)) != 0
        trunc = ((flags & L.F_TIMEOUT) != 0) & ~hard
        free = sum(int((r[5]["control"] == 0).sum()) for r in runs)
        cut = sum(float(r[4]["cut"].sum()) for r in runs)
        print("boot: %d truncated and %d hard-ended blocks, %d uncontrolled rows, %d cut rows" % (trunc.sum(), hard.sum(), free, cut))
        assert trunc.any() and hard.any() and free > 0 and cut > 0
    if name.startswith("ragged"):
        assert set(runs[0][4]["n"].reshape(-1).tolist()) == {35.0}
