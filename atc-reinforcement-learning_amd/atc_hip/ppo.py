"""A PPO collection in three calls on fixed shapes: AtcVecEnv.rollout_policy (or rollout_policy_traffic) -> one value forward ->
AtcVecEnv.gae.  The collection loop and the advantage recurrence each run inside one launch (include/atc_step.h: atc_rollout_policy,
atc_gae); the value network runs as one batched forward over the rows the decisions saw — any callable of the trainer's, or critic(env,
weights): the library's own forward of a critic packed by atc_hip.value (atc_value_forward).
collect_bootstrap() also bootstraps time-limit ends (atc_rollout_policy_ends, atc_gae_boot: the terminal observations join the one
value forward) and returns the mask of the aircraft each decision controlled.
policy_grad() is the policy half of the update on such a collection: the clipped surrogate loss and its gradient with respect to the
packed weights in one call (atc_ppo_policy_grad), and value_grad() the value half: the clipped value loss of the packed critic and its
gradient (atc_ppo_value_grad).  update() closes the iteration: the advantages normalised once per collection (atc_adv_normalise), then per
minibatch the two gradient calls and ONE optimiser step on both packed tensors (atc_adam_step: the gradient-norm clip over both, the entropy
term on log_std, Adam), with adam_state() holding the moments and every buffer.  An iteration then touches neither autograd nor torch.optim,
and update() reads no device value on the host.  (policy_grad(normalise=True) on its own still makes its three reductions in torch.)
collect_bootstrap_traffic() is collect_bootstrap() for a policy that sees traffic: atc_rollout_policy_term stores the records of the
terminal states next to their observations, and both join the one value forward.
Not covered, the trainer's: learning-rate or clip-range schedules, which are update()'s arguments from call to call."""
from . import layout as L
from . import policy as _policy


def value_rows(env, rollout, obs0, hold=1, traffic=0):
    """The value network's input, [D + 1, B, N, IN]: row d < D is the row decision d saw — obs0 for d = 0, the observation step
    d * hold - 1 stored otherwise, widened by the stored traffic records with traffic=K (atc_hip.policy.input_rows) — and row D the last
    stored observation, with traffic the records of the state the env is in NOW, obtained with observe_traffic()."""
    torch = env.torch
    obs = rollout["obs"]
    T, B, N = int(obs.shape[0]), env.B, env.N
    D = T // hold
    own = torch.empty((D + 1, B, N, L.OBS_DIM), dtype=obs.dtype, device=obs.device)
    own[0] = obs0.reshape(B, N, L.OBS_DIM)
    own[1:] = obs.reshape(D, hold, B, N, L.OBS_DIM)[:, hold - 1]
    if not traffic:
        return own
    records = torch.cat([rollout["traffic"], env.observe_traffic().reshape((1,) + tuple(rollout["traffic"].shape[1:]))], dim=0)
    return _policy.input_rows(own, records)


def truncated(term_flags):
    """[D, B] uint8 from rollout_policy_ends()'s term_flags: 1 where the block's ending step is a time-limit end — ATC_F_TIMEOUT set
    with ATC_F_BELOW_MVA, ATC_F_OUTSIDE and ATC_F_CONFLICT clear among the env's aircraft — which gae_boot() bootstraps."""
    import torch
    f = term_flags.to(torch.int32)
    hit = ((f & L.F_TIMEOUT) != 0) & ((f & (L.F_BELOW_MVA | L.F_OUTSIDE | L.F_CONFLICT)) == 0)
    return hit.to(torch.uint8).contiguous()


def collect(env, weights, value_fn, T, hold=1, traffic=0, gamma=0.99, lam=0.95, seed=0, decision0=0, obs0=None, per_decision=False):
    """One on-policy collection of T steps, D = T // hold decisions, in three calls, in this order:
      1. env.rollout_policy(weights, T, hold, seed, decision0, obs0=obs0) — env.rollout_policy_traffic with traffic=K;
      2. values = value_fn(x): ONE forward over x = value_rows(...), [D + 1, B, N, IN] float32 with IN = 10 + 7 K — the stacked input
         rows of the D decisions plus the last observation; it returns [D + 1, B, NV] or [D + 1, B] (made contiguous float32 here);
      3. env.gae(reward, done, values, hold, gamma, lam, per_decision=per_decision).
    With traffic=K the value input of rows 0 .. D - 1 is atc_hip.policy.input_rows of what the decisions saw; the final state's row takes
    the own words of the last stored observation, and its traffic records are obtained with observe_traffic() on the state the rollout
    left, so the env must have been made with AtcVecEnv(traffic=K); which of the columns the critic reads is value_fn's choice.
    obs0 defaults to the env's bound observation tensor, as in rollout_policy; a copy is taken before the launch overwrites it.
    Returns the rollout's dict plus "values", "adv", "ret", "block_reward", "block_done" and "block_steps" (AtcVecEnv.gae).  The copy of
    obs0 that decision 0 saw is kept on the env for policy_grad(), next to the collection's obs tensor it belongs to.
    Every done is a terminal state here; collect_bootstrap() bootstraps the time-limit ends."""
    return _collect(env, weights, value_fn, T, hold, traffic, gamma, lam, seed, decision0, obs0, per_decision, False)


def collect_bootstrap(env, weights, value_fn, T, hold=1, traffic=0, gamma=0.99, lam=0.95, seed=0, decision0=0, obs0=None, per_decision=False):
    """collect() that treats time-limit ends as truncations, in the same three calls:
      1. env.rollout_policy_ends(weights, T, 0, hold, seed, decision0, obs0=obs0);
      2. ONE forward over [2 D + 1, B, N, 10]: collect()'s D + 1 rows, then rows D + 1 .. 2 D = term_obs (zeros where a block did not
         end its episode); the result is split into values [D + 1, ...] and boot [D, ...];
      3. env.gae_boot(reward, done, values, boot, truncated(term_flags), hold, gamma, lam, per_decision=per_decision).
    Returns collect()'s dict plus "term_obs", "term_flags", "control" (the rollout's), "boot" and "trunc".
    traffic=K raises ValueError: the traffic records of a terminal state are not produced, so a critic that reads them cannot be
    evaluated there — next to advantage normalisation the one thing left to the trainer."""
    if int(traffic):
        raise ValueError("collect_bootstrap() is for traffic=0: the traffic records of a terminal state are not produced")
    return _collect(env, weights, value_fn, T, hold, 0, gamma, lam, seed, decision0, obs0, per_decision, True)


def collect_bootstrap_traffic(env, weights, value_fn, T, traffic, hold=1, gamma=0.99, lam=0.95, seed=0, decision0=0, obs0=None, per_decision=False):
    """collect_bootstrap() for a policy that sees traffic (traffic=K: 1, 2 or 4), in the same three calls:
      1. env.rollout_policy_term(weights, T, K, hold, seed, decision0, obs0=obs0), which also stores term_traffic, the records of the
         state each ended block's episode ended in;
      2. ONE forward over [2 D + 1, B, N, 10 + 7 K]: value_rows(..., traffic=K)'s D + 1 rows, then rows D + 1 .. 2 D =
         atc_hip.policy.input_rows(term_obs, term_traffic) (zeros where a block did not end its episode); the result is split into
         values [D + 1, ...] and boot [D, ...];
      3. env.gae_boot(reward, done, values, boot, truncated(term_flags), hold, gamma, lam, per_decision=per_decision), which reads boot
         only where trunc is set.
    The env must have been made with AtcVecEnv(traffic=K), as for collect(traffic=K).  Returns collect_bootstrap()'s dict plus "traffic" and
    "term_traffic"; policy_grad(), value_grad() and update() take it as they take collect(traffic=K)'s."""
    K = int(traffic)
    if K not in L.POLICY_TRAFFIC_K:
        raise ValueError("collect_bootstrap_traffic() is for traffic in %s; collect_bootstrap() bootstraps the ten-word policy" % (L.POLICY_TRAFFIC_K,))
    return _collect(env, weights, value_fn, T, hold, K, gamma, lam, seed, decision0, obs0, per_decision, True)


def _collect(env, weights, value_fn, T, hold, traffic, gamma, lam, seed, decision0, obs0, per_decision, bootstrap):
    torch = env.torch
    K = int(traffic)
    if K and env.traffic_k != K:
        raise ValueError("collect(traffic=%d) needs an env made with AtcVecEnv(traffic=%d): the last row's records come from observe_traffic()" % (K, K))
    x0 = (env.obs if obs0 is None else obs0).clone()
    if K and bootstrap:
        out = env.rollout_policy_term(weights, T, K, hold=hold, seed=seed, decision0=decision0, obs0=x0)
    elif K:
        out = env.rollout_policy_traffic(weights, T, K, hold=hold, seed=seed, decision0=decision0, obs0=x0)
    elif bootstrap:
        out = env.rollout_policy_ends(weights, T, 0, hold=hold, seed=seed, decision0=decision0, obs0=x0)
    else:
        out = env.rollout_policy(weights, T, hold=hold, seed=seed, decision0=decision0, obs0=x0)
    env._collected_obs0 = (out["obs"], x0)      # what decision 0 saw, for policy_grad() on this collection
    rows = value_rows(env, out, x0, hold=hold, traffic=K)
    if bootstrap:
        term = _policy.input_rows(out["term_obs"], out["term_traffic"]) if K else out["term_obs"]
        rows = torch.cat([rows, term.reshape((-1,) + tuple(rows.shape[1:]))], dim=0)
    with torch.no_grad():
        values = value_fn(rows)
    values = values.to(dtype=torch.float32).contiguous()
    if not bootstrap:
        res = dict(out, values=values)
        res.update(env.gae(out["reward"], out["done"], values, hold=hold, gamma=gamma, lam=lam, per_decision=per_decision))
        return res
    D = int(rows.shape[0]) // 2
    values, boot = values[:D + 1].contiguous(), values[D + 1:].contiguous()
    trunc = truncated(out["term_flags"])
    res = dict(out, values=values, boot=boot, trunc=trunc)
    res.update(env.gae_boot(out["reward"], out["done"], values, boot, trunc, hold=hold, gamma=gamma, lam=lam, per_decision=per_decision))
    return res



def policy_grad(env, collected, weights, index=None, clip=0.2, normalise=True, workgroups=0, out=None):
    """The PPO policy loss and gradient on a collection (AtcVecEnv.ppo_policy_grad), from the dict collect() / collect_bootstrap() return —
    the row decision 0 saw is the copy that call kept on `env`, so it must be `env`'s latest collection — or from one put together by hand:
    "obs0", "obs", "action", "logp", "adv" (and "traffic", "control" where the rollout stored them).
    The D * B * N source rows are flat views, nothing is copied: the rows the decisions saw are value_rows(...)[:-1] (obs0, then the
    observation each block's last step stored), "traffic" the records next to them (the policy sees K = traffic.shape[-2] of them),
    "action" and "logp" as stored; adv is [D, B, N], or a per-env [D, B] / [D, B, 1] expanded over the env's aircraft.
    mask = "control" where the dict has it: an aircraft that was not under control takes no part.  index: int32 [R] or None, the
    minibatch (torch.randperm(D * B * N, dtype=torch.int32, device=...)[a:b]).  normalise=True: shift and scale are the mean and
    1 / (std + 1e-8) of adv over the controlled rows of the whole collection, three torch reductions; False passes 0 and 1.
    Returns ppo_policy_grad's dict: "grad" (to be assigned to weights.grad), "stats", "logp"."""
    torch = env.torch
    action = collected["action"]
    D, B, N = int(action.shape[0]), env.B, env.N
    hold = int(collected["obs"].shape[0]) // D
    obs0 = collected.get("obs0")
    if obs0 is None:
        kept = getattr(env, "_collected_obs0", None)
        if kept is None or kept[0] is not collected["obs"]:
            raise ValueError("collected is not this env's latest collect() / collect_bootstrap(): give the row decision 0 saw as collected['obs0']")
        obs0 = kept[1]
    own = value_rows(env, collected, obs0, hold=hold)[:-1]
    adv = collected["adv"]
    if adv.dim() == 2 or int(adv.shape[-1]) != N:
        if adv.dim() == 3 and int(adv.shape[-1]) != 1:
            raise ValueError("adv must be [D, B, N], or per env [D, B] / [D, B, 1]")
        adv = adv.reshape(D, B, 1).expand(D, B, N).contiguous()
    control = collected.get("control")
    shift, scale = 0.0, 1.0
    if normalise:
        a = adv if control is None else adv[control.bool()]
        shift, scale = float(a.mean()), float(1.0 / (a.std() + 1e-8))
    return env.ppo_policy_grad(weights, own, action, collected["logp"], adv, traffic=collected.get("traffic"), mask=control, index=index, clip=clip,
                               adv_shift=shift, adv_scale=scale, workgroups=workgroups, out=out)


def mc_returns(env, w, M, K, H, gamma, *, seed=0, decision0=0, obs0=None, first=None):
    """Monte-Carlo return of the packed policy `w` from the state the env is in NOW, [B]: the mean over M continuations, flown on copies of
    the state in one launch (AtcVecEnv.lookahead_policy, which writes no state), of the discounted segment rewards seg[m, 0] + gamma seg[m, 1]
    + ... (atc_hip.shield.discounted; gamma is per DECISION of K steps) — a target for V(s), a check of the critic, the leaf value of a tree
    of branch() / select().  first: [M, B, N, 3] fixes the first decision of every continuation, which makes the mean an estimate of Q(s, a)
    for first[m] = a.  A continuation that was not evaluated (n_steps == 0) enters with its zeros."""
    from . import shield
    look = env.lookahead_policy(w, K, H, first=first, M=None if first is not None else M, seed=seed, decision0=decision0, obs0=obs0, outputs=())
    return shield.discounted(look["seg_reward"], gamma).mean(dim=0)


def critic(env, weights):
    """A value_fn for collect() / collect_bootstrap() that runs the library's critic: env.value_forward(weights, rows) on the rows it is
    given, [D + 1, B, N, IN] or [2 D + 1, B, N, IN] -> one value per aircraft.  weights: the tensor of atc_hip.value.pack_mlp(traffic=K) for
    the K of the collection (collect(traffic=K) hands it rows of 10 + 7 K words)."""
    def value_fn(rows):
        return env.value_forward(weights, rows.contiguous())
    return value_fn


def value_grad(env, collected, weights, index=None, clip=0.2, workgroups=0, out=None):
    """The PPO value loss and gradient on a collection (AtcVecEnv.ppo_value_grad), from the dict collect() / collect_bootstrap() return, or
    from one put together by hand, as policy_grad() takes it: "obs0" (or the copy the collection kept on `env`), "obs", "action", "values",
    "ret" (and "traffic", "control" where the rollout stored them).
    v_old = values[:-1] and ret, both [D, B, N] — a per-env [D, B] or [D, B, 1] is expanded over the env's aircraft —; the rows are
    value_rows(...)[:-1], "traffic" the records next to them, mask = "control", index the int32 minibatch; nothing else is copied.
    The critic is packed for the collection's K (atc_hip.value.pack_mlp(traffic=K), K = collected["traffic"].shape[-2]) or for K = 0: a
    critic that reads the own row only, to which the stored records are not passed.  Any other size: ValueError, before any call on `env`.
    Returns ppo_value_grad's dict: "grad" (to be assigned to weights.grad), "stats", "value"."""
    action = collected["action"]
    D, B, N = int(action.shape[0]), env.B, env.N
    traffic = _critic_traffic(collected, weights)
    hold = int(collected["obs"].shape[0]) // D
    obs0 = collected.get("obs0")
    if obs0 is None:
        kept = getattr(env, "_collected_obs0", None)
        if kept is None or kept[0] is not collected["obs"]:
            raise ValueError("collected is not this env's latest collect() / collect_bootstrap(): give the row decision 0 saw as collected['obs0']")
        obs0 = kept[1]
    own = value_rows(env, collected, obs0, hold=hold)[:-1]

    def per_aircraft(v, name):
        if v.dim() == 3 and int(v.shape[-1]) == N:
            return v.contiguous()
        if v.dim() == 3 and int(v.shape[-1]) != 1:
            raise ValueError("%s must be [D, B, N], or per env [D, B] / [D, B, 1]" % name)
        return v.reshape(D, B, 1).expand(D, B, N).contiguous()
    return env.ppo_value_grad(weights, own, per_aircraft(collected["values"][:-1], "values[:-1]"), per_aircraft(collected["ret"], "ret"),
                              traffic=traffic, mask=collected.get("control"), index=index, clip=clip, workgroups=workgroups, out=out)


def _critic_traffic(collected, vw):
    """The records value_grad() passes next to the rows: the collection's where the critic is packed for its K, None for a K = 0 critic"""
    traffic = collected.get("traffic")
    K = 0 if traffic is None else int(traffic.shape[-2])
    if int(vw.numel()) == L.value_words(K):
        return traffic
    if int(vw.numel()) == L.value_words(0):
        return None
    raise ValueError("the critic must be packed for the collection's K = %d (atc_hip.value.pack_mlp(traffic=%d): %d words) or for K = 0 (%d words), "
                     "got %d words" % (K, K, L.value_words(K), L.value_words(0), int(vw.numel())))


def adam_state(env, w, vw=None):
    """What update() keeps from call to call for the packed policy `w` and, where given, the packed critic `vw`: zeroed first and second
    moments per tensor ("m", "v": lists in the order policy, critic), the update count "t" = 0, and every out= buffer of the calls update()
    makes, allocated once — those whose size depends on the collection are made by the first update() that meets that size and kept."""
    torch = env.torch
    tensors = [w] if vw is None else [w, vw]
    for t in tensors:
        if not (torch.is_tensor(t) and t.dtype == torch.float32 and t.dim() == 1 and t.is_contiguous()):
            raise ValueError("w and vw must be contiguous 1-D float32 tensors (atc_hip.policy.pack_mlp, atc_hip.value.pack_mlp)")
    new = lambda *shape, **kw: torch.empty(shape, dtype=kw.get("dtype", torch.float32), device=w.device)      # noqa: E731
    return {"t": 0, "m": [torch.zeros_like(t) for t in tensors], "v": [torch.zeros_like(t) for t in tensors],
            "grad": [new(int(t.numel())) for t in tensors],
            "scratch": [new(L.PPO_GRAD_DEFAULT_WG, int(t.numel()) + L.PPO_GRAD_STATS) for t in tensors],
            "rows": {}, "adv": {}}


def update(env, collected, w, vw, state, *, epochs=4, minibatches=4, clip=0.2, vclip=0.2, lr=3e-4, ent_coef=0.0, vf_coef=0.5, max_grad_norm=0.5,
           eps=1e-5, perm=None, seed=0):
    """The update half of a PPO iteration on a collection, with no torch op between the library's calls and no device value read on the host:
      once:          env.adv_normalise(adv, mask=collected.get("control")) — a per-env [D, B] adv expanded over the aircraft as in policy_grad();
      per epoch e:   one int32 permutation of the D * B * N rows: perm[e] if given (an int32 tensor [E, R] or a list of [R] tensors on the
                     env's device), else torch.randperm on the device from a generator seeded with (seed, e);
      per minibatch: policy_grad(..., normalise=False) on a shallow copy of `collected` whose "adv" is the normalised tensor, value_grad(),
                     then ONE env.adam_step over both tensors with step = state["t"] + 1: the critic's gradient scaled by vf_coef, -ent_coef
                     added to the three log_std words, the norm over both clipped to max_grad_norm.
    w and vw are updated in place; state is adam_state(env, w, vw)'s and carries the moments and the count.  w is packed for the collection's
    K (the K of collected["traffic"], 0 without it), vw for that K or for K = 0 — a critic that reads the own row only: value_grad() then
    passes it no records; any other pair raises ValueError before any call reaches the env.  The minibatches are the
    `minibatches` consecutive slices of the permutation ([k R // M, (k + 1) R // M)).
    Returns {"policy_stats" [E, M, 8], "value_stats" [E, M, 8], "adam_stats" [E, M, 4], "adv_stats" [4]} as device tensors."""
    torch = env.torch
    action = collected["action"]
    D, B, N = int(action.shape[0]), env.B, env.N
    R = D * B * N
    E, M = int(epochs), int(minibatches)
    if E < 1 or not 1 <= M <= R:
        raise ValueError("epochs must be >= 1 and minibatches 1 .. the number of rows")
    if len(state["m"]) != 2:
        raise ValueError("state must be adam_state(env, w, vw) of both tensors")
    K = {L.policy_words(k): k for k in (0,) + L.POLICY_TRAFFIC_K}.get(int(w.numel()))
    if K is None:
        raise ValueError("w is not a packed policy (atc_hip.policy.pack_mlp)")
    tr = collected.get("traffic")
    if K != (0 if tr is None else int(tr.shape[-2])):
        raise ValueError("the policy must be packed for the collection's K = %d (atc_hip.policy.pack_mlp(traffic=%d)), got one for K = %d" % (
            0 if tr is None else int(tr.shape[-2]), 0 if tr is None else int(tr.shape[-2]), K))
    _critic_traffic(collected, vw)
    if perm is not None and len(perm) < E:
        raise ValueError("perm must hold one permutation per epoch")
    adv = collected["adv"]
    if adv.dim() == 2 or int(adv.shape[-1]) != N:
        if adv.dim() == 3 and int(adv.shape[-1]) != 1:
            raise ValueError("adv must be [D, B, N], or per env [D, B] / [D, B, 1]")
        adv = adv.reshape(D, B, 1).expand(D, B, N).contiguous()
    dev = adv.device
    abuf = state["adv"].get((D, B, N))
    if abuf is None:
        abuf = state["adv"][(D, B, N)] = {"adv": torch.empty((D, B, N), dtype=torch.float32, device=dev), "stats": torch.empty(L.ADV_STATS, dtype=torch.float32, device=dev),
                                          "scratch": torch.empty((L.adv_workgroups(R), 3), dtype=torch.float64, device=dev)}
    normed = env.adv_normalise(adv, collected.get("control"), out=abuf)
    mb = dict(collected, adv=normed["adv"])
    res = {"policy_stats": torch.empty((E, M, L.PPO_GRAD_STATS), dtype=torch.float32, device=dev),
           "value_stats": torch.empty((E, M, L.PPO_VALUE_STATS), dtype=torch.float32, device=dev),
           "adam_stats": torch.empty((E, M, L.ADAM_STATS), dtype=torch.float32, device=dev), "adv_stats": normed["stats"].clone()}
    add = (_policy.offsets(K)["log_std"][0], 3, -float(ent_coef))
    for e in range(E):
        if perm is not None:
            order = perm[e]
        else:
            gen = torch.Generator(device=dev)
            gen.manual_seed(((int(seed) & 0xffffffff) << 24) + e)
            order = torch.randperm(R, generator=gen, dtype=torch.int32, device=dev)
        for k in range(M):
            index = order[k * R // M:(k + 1) * R // M]
            n = int(index.numel())
            G = L.ppo_grad_workgroups(n)
            rows = state["rows"].get(n)
            if rows is None:
                rows = state["rows"][n] = (torch.empty(n, dtype=torch.float32, device=dev), torch.empty(n, dtype=torch.float32, device=dev))
            policy_grad(env, mb, w, index=index, clip=clip, normalise=False,
                        out={"grad": state["grad"][0], "stats": res["policy_stats"][e, k], "logp": rows[0], "scratch": state["scratch"][0][:G]})
            value_grad(env, collected, vw, index=index, clip=vclip,
                       out={"grad": state["grad"][1], "stats": res["value_stats"][e, k], "value": rows[1], "scratch": state["scratch"][1][:G]})
            state["t"] += 1
            env.adam_step([{"w": w, "grad": state["grad"][0], "m": state["m"][0], "v": state["v"][0], "add": add},
                           {"w": vw, "grad": state["grad"][1], "m": state["m"][1], "v": state["v"][1], "grad_scale": vf_coef}],
                          lr=lr, step=state["t"], eps=eps, max_norm=max_grad_norm, out=res["adam_stats"][e, k])
    return res
