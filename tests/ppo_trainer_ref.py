"""An independent PPO trainer in plain torch on the CPU: torch.autograd, torch.nn.utils.clip_grad_norm_ and torch.optim.Adam on the stored
arrays of a collection.  TEST INFRASTRUCTURE ONLY; needs no GPU.  What atc_hip/ppo.py composes out of library calls (collect /
collect_bootstrap, policy_grad, value_grad, update) is held to it by tests/test_z_ppo_iteration.py.

It shares no code with the restatements written in the kernels' order (ppo_grad_ref, ppo_value_ref's evaluate, ppo_update_ref, gae_ref,
gae_boot_ref): only policy_ref.split / ppo_value_ref.split unpack the weights.  Everything is computed from the header's definitions
(include/atc_step.h), in `dtype`: torch.float64 is the reference, torch.float32 the twin that sets the bars (4 x the twin's deviation from
the reference on the same collection).

  Trainer(w, vw, K, dtype, KV=None, **hyper)     parameters and ONE optimiser, carried from iteration to iteration
  Trainer.iterate(stored, perm, hold, ...)       one iteration on the stored arrays of one collection -> a dict, see there
  Trainer.weights()                              (w, vw) packed, as numpy arrays of `dtype`

Parameters that the library holds as float32 words (gamma, lam, clip, vclip, vf_coef, ent_coef, the 1e-8 of the normalisation) enter rounded
to float32, as inputs; lr, Adam's eps and betas and max_grad_norm are doubles there and enter as given."""
import math

import numpy as np
import torch

import policy_ref as P
import ppo_value_ref as PV

F_BELOW_MVA, F_OUTSIDE, F_TIMEOUT, F_CONFLICT = 1, 2, 8, 64      # include/atc_step.h: ATC_F_*
LOG_2PI = math.log(2.0 * math.pi)


def _f32(x):
    return float(np.float32(x))


def _mlp(p, x):
    h = torch.tanh(x @ p["W1"].T + p["b1"])
    h = torch.tanh(h @ p["W2"].T + p["b2"])
    return h @ p["W3"].T + p["b3"]


class Trainer:
    def __init__(self, w, vw, K=0, dtype=torch.float64, KV=None, lr=3e-4, eps=1e-5, clip=0.2, vclip=0.2, ent_coef=0.0, vf_coef=0.5, max_grad_norm=0.5,
                 gamma=0.99, lam=0.95):
        """w, vw: the packed float32 policy (traffic K) and critic (traffic KV, default K; 0 with K > 0: a critic that reads the own row only)"""
        self.K, self.KV, self.dtype = int(K), int(K if KV is None else KV), dtype
        t = lambda a: torch.nn.Parameter(torch.tensor(np.array(a, np.float64), dtype=dtype))      # noqa: E731
        self.pi = {k: t(v) for k, v in P.split(np.asarray(w), self.K).items()}
        self.vf = {k: t(v) for k, v in PV.split(np.asarray(vw), self.KV).items()}
        self.params = list(self.pi.values()) + list(self.vf.values())
        self.opt = torch.optim.Adam(self.params, lr=lr, eps=eps)
        self.clip, self.vclip, self.ent_coef, self.vf_coef = _f32(clip), _f32(vclip), _f32(ent_coef), _f32(vf_coef)
        self.gamma, self.lam, self.max_grad_norm = _f32(gamma), _f32(lam), float(max_grad_norm)
        self.steps = 0

    def weights(self):
        cat = lambda d: torch.cat([v.detach().reshape(-1) for v in d.values()]).numpy().copy()      # noqa: E731
        return cat(self.pi), cat(self.vf)

    def _t(self, a):
        return torch.tensor(np.asarray(a, np.float64), dtype=self.dtype)

    def rows(self, stored, hold):
        """[D + 1, B, N, 10 + 7 K]: row d what decision d saw — obs0, then the observation step d hold - 1 stored — and row D the last
        observation; traffic=K widens a row by words 0..6 of each of its K records (row D: the final records)"""
        obs = np.asarray(stored["obs"])
        B, N = np.asarray(stored["action"]).shape[1:3]
        T = obs.shape[0]
        D = T // hold
        obs = obs.reshape(T, B, N, 10)
        own = [np.asarray(stored["obs0"]).reshape(B, N, 10)] + [obs[d * hold - 1] for d in range(1, D)] + [obs[T - 1]]
        x = np.stack(own)
        if self.K:
            rec = np.concatenate([np.asarray(stored["traffic"]), np.asarray(stored["traffic_final"]).reshape((1, B, N, self.K, 8))])
            x = np.concatenate([x, rec[..., :7].reshape(D + 1, B, N, 7 * self.K)], axis=-1)
        return self._t(x)

    def _v(self, x):
        return _mlp(self.vf, x[..., :10 + 7 * self.KV])[..., 0]

    def gae(self, stored, values, boot, hold, per_decision):
        """(adv, ret) [D, B, NV...] by a plain backward loop; values [D + 1, B(, N)], boot [D, B(, N)] or None (no bootstrap)"""
        reward, done = self._t(stored["reward"]), np.asarray(stored["done"]) != 0
        T, B = reward.shape
        D = T // hold
        wide = values.dim() == 3
        col = (lambda a: a[:, None]) if wide else (lambda a: a)
        trunc = None
        if boot is not None:
            f = np.asarray(stored["term_flags"]).astype(np.int64)
            trunc = ((f & F_TIMEOUT) != 0) & ((f & (F_BELOW_MVA | F_OUTSIDE | F_CONFLICT)) == 0)
        gamma, lam = self.gamma, self.lam
        G = gamma if per_decision else gamma ** hold
        adv = torch.zeros_like(values[:-1])
        a_next = torch.zeros_like(values[0])
        for d in range(D - 1, -1, -1):
            R = torch.zeros(B, dtype=self.dtype)
            alive = np.ones(B, bool)
            steps = np.zeros(B, np.int64)
            for j in range(hold):
                t = d * hold + j
                R = R + torch.tensor(alive) * reward[t] * (1.0 if per_decision else gamma ** j)
                steps += alive
                alive = alive & ~done[t]      # the first done ends the block: what lies behind it belongs to the next episode
            term = torch.tensor(~alive)
            cont = col(R) + G * values[d + 1] - values[d] + G * lam * a_next
            end = col(R) - values[d]
            if trunc is not None:
                Gn = torch.tensor(np.full(B, gamma) if per_decision else gamma ** steps.astype(np.float64), dtype=self.dtype)
                end = torch.where(col(torch.tensor(trunc[d])), col(R) + col(Gn) * boot[d] - values[d], end)
            a = torch.where(col(term), end, cont)
            adv[d] = a
            a_next = a
        return adv, adv + values[:-1]

    def iterate(self, stored, perm, hold=1, epochs=None, minibatches=1, per_decision=False, bootstrap=False, per_env=False):
        """One iteration on the stored arrays of a collection: "obs0" [B, N, 10], "obs" [T, B, N * 10], "action" [D, B, N, 3], "logp" [D, B, N],
        "reward", "done" [T, B]; with K > 0 "traffic" [D, B, N, K, 8] and "traffic_final" [B, N, K, 8]; with bootstrap "term_obs" [D, B, N, 10]
        and "term_flags" [D, B]; "control" [D, B, N] where the collection has it.  perm: [E, R] integers.  per_env: the collection's values
        are the mean of the critic over an env's aircraft, [D + 1, B], and so are adv and ret (expanded over the aircraft in the update).
        Returns {"values", "adv", "ret", "adv_norm", "adv_n", "adv_mean", "adv_std", per minibatch [E, M]: "n", "policy_loss", "value_loss",
        "loss", "kl", "ratio", "cut", "vcut" (counts), "norm", "coef", "dlogp_max"; "w", "vw": the weights after the iteration; "margins":
        {"ratio", "adv", "vclip", "vtie"}, the smallest over every participating row of every minibatch}."""
        D, B, N = np.asarray(stored["action"]).shape[:3]
        R = D * B * N
        E = len(perm) if epochs is None else int(epochs)
        M = int(minibatches)
        x = self.rows(stored, hold)
        with torch.no_grad():
            values = self._v(x)
            boot = self._v(self._t(np.asarray(stored["term_obs"]).reshape(D, B, N, 10))) if bootstrap else None
            if per_env:
                values, boot = values.mean(-1), None if boot is None else boot.mean(-1)
            adv, ret = self.gae(stored, values, boot, hold, per_decision)
        wide = (lambda a: a[..., None].expand(D, B, N)) if per_env else (lambda a: a)
        ctrl = torch.ones((D, B, N), dtype=torch.bool) if stored.get("control") is None else torch.tensor(np.asarray(stored["control"]) != 0)
        sel = wide(adv)[ctrl]
        mean, std = sel.mean(), sel.std(unbiased=True)
        a_norm = (wide(adv) - mean) * (1.0 / (std + _f32(1e-8)))
        out = {"values": values, "adv": adv, "ret": ret, "adv_norm": torch.where(ctrl, a_norm, torch.zeros_like(a_norm)), "adv_n": int(ctrl.sum()),
               "adv_mean": float(mean), "adv_std": float(std)}
        rows, act, lp_old = x[:-1].reshape(R, -1), self._t(stored["action"]).reshape(R, 3), self._t(stored["logp"]).reshape(R)
        A_all, v_old_all, ret_all, c_all = a_norm.reshape(R), wide(values[:-1]).reshape(R), wide(ret).reshape(R), ctrl.reshape(R)
        names = ("n", "policy_loss", "value_loss", "loss", "kl", "ratio", "cut", "vcut", "norm", "coef", "dlogp_max")
        st = {k: np.zeros((E, M)) for k in names}
        marg = {"ratio": np.inf, "adv": np.inf, "vclip": np.inf, "vtie": np.inf}
        clip, vclip = self.clip, self.vclip
        for e in range(E):
            order = torch.as_tensor(np.asarray(perm[e]).astype(np.int64))
            for k in range(M):
                idx = order[k * R // M:(k + 1) * R // M]
                idx = idx[c_all[idx]]
                n = int(idx.numel())
                mu = _mlp(self.pi, rows[idx][:, :10 + 7 * self.K])
                ls = self.pi["log_std"]
                z = (act[idx] - mu) / torch.exp(ls)
                logp = (-0.5 * z * z - ls).sum(-1) - 1.5 * LOG_2PI
                ratio = torch.exp(logp - lp_old[idx])
                A = A_all[idx]
                pl = (-torch.minimum(ratio * A, torch.clamp(ratio, 1.0 - clip, 1.0 + clip) * A)).sum() / n
                v = self._v(rows[idx])
                v_old, rt = v_old_all[idx], ret_all[idx]
                vc = v_old + torch.clamp(v - v_old, -vclip, vclip)
                e2, ec2 = (v - rt) ** 2, (vc - rt) ** 2
                vl = (0.5 * torch.maximum(e2, ec2)).sum() / n
                loss = pl + self.vf_coef * vl - self.ent_coef * ls.sum()
                self.opt.zero_grad()
                loss.backward()
                norm = float(torch.nn.utils.clip_grad_norm_(self.params, self.max_grad_norm)) if 0.0 < self.max_grad_norm < math.inf else \
                    float(torch.sqrt(sum((p.grad ** 2).sum() for p in self.params)))
                self.opt.step()
                self.steps += 1
                with torch.no_grad():
                    r, dv = ratio.detach(), (v - v_old).detach()
                    cut = ((A >= 0) & (r > 1.0 + clip)) | ((A < 0) & (r < 1.0 - clip))
                    outside = dv.abs() > vclip
                    vcut = outside & (e2 < ec2)
                    coef = min(1.0, self.max_grad_norm / (norm + 1e-6)) if 0.0 < self.max_grad_norm < math.inf else 1.0
                    for name, val in (("n", n), ("policy_loss", pl), ("value_loss", vl), ("loss", loss), ("kl", (lp_old[idx] - logp).sum() / n),
                                      ("ratio", r.sum() / n), ("cut", cut.sum()), ("vcut", vcut.sum()), ("norm", norm), ("coef", coef),
                                      ("dlogp_max", (logp - lp_old[idx]).abs().max())):
                        st[name][e, k] = float(val)
                    marg["ratio"] = min(marg["ratio"], float(torch.minimum((r - (1.0 - clip)).abs(), (r - (1.0 + clip)).abs()).min()))
                    marg["adv"] = min(marg["adv"], float(A.abs().min()))
                    marg["vclip"] = min(marg["vclip"], float((dv.abs() - vclip).abs().min()))
                    if bool(outside.any()):
                        marg["vtie"] = min(marg["vtie"], float(((e2 - ec2).abs() / torch.maximum(e2, ec2))[outside].min()))
        out.update(st)
        out = {k: (v.detach().numpy().copy() if torch.is_tensor(v) else v) for k, v in out.items()}
        out["w"], out["vw"] = self.weights()
        out["margins"] = marg
        out["steps"] = self.steps
        return out
