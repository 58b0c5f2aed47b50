"""Agent — a packed policy (atc_hip.policy) behind stable-baselines' `model.predict`, for the reference's deployment loop

    agent = Agent(atc_hip.checkpoint.load("policy.npz")["policy"])
    obs = env.reset()
    while True:
        action, _ = agent.predict(obs)
        obs, reward, done, info = env.step(action)
        env.render()

on the drop-in AtcGym (one observation of 10 words) or an AtcSBVecEnv (rows of [N * 10 | N * K * 7] words per env).  numpy in, numpy out;
the decision itself is AtcVecEnv.policy_forward (atc_policy_forward, include/atc_step.h): the rollout's arithmetic and the rollout's draws."""
import numpy as np

from . import layout as L
from . import lib as _lib
from . import policy
from .vec_env import AtcVecEnv


class _Host:
    """what AtcVecEnv.policy_forward reads of an env: the device, the library, a sector handle (which names the device only) and the stream"""

    def __init__(self, device):
        from envs.atc import scenarios
        self.torch = _lib._torch_cuda()
        self.sector = _lib.Scenario(scenarios.compile_scenario(scenarios.LOWW(), grid_cell=None), device)
        self.device = self.sector.device
        self._lib = _lib.load()

    def _stream(self):
        return _lib.current_stream_ptr(self.device)


class Agent:
    def __init__(self, weights, device=0, seed=0):
        """weights: a packed policy (tensor or array of L.policy_words(K) float32 words; K, the traffic records per aircraft it sees, is found
        from its size); a copy is kept on `device`.  seed: the key of the draws; `decision` counts the calls of predict()."""
        self._host = _Host(device)
        torch = self._host.torch
        w = torch.as_tensor(np.asarray(weights.detach().cpu()) if torch.is_tensor(weights) else np.asarray(weights))
        if w.dtype != torch.float32:
            raise ValueError("packed weights are float32, got %s" % w.dtype)
        self.traffic = policy.traffic_of(w.numel())
        self.weights = w.reshape(-1).to(self._host.device).contiguous()
        self.seed = int(seed)
        self.decision = 0

    def predict(self, obs, state=None, mask=None, deterministic=False):
        """stable-baselines' BaseRLModel.predict: (actions, None).  obs: [10] (AtcGym) -> actions [3]; [n_envs, N * 10 + N * K * 7]
        (AtcSBVecEnv, K = the policy's traffic records) -> actions [n_envs, N * 3], clamped to [-1, 1].  Each call is one decision of the
        rollout's key sequence (seed, decision, aircraft row), so successive calls draw fresh noise; deterministic=True returns the mean's
        clamp and leaves the counter alone.  state and mask are the recurrent policies' and are not read."""
        torch, dev, K = self._host.torch, self._host.device, self.traffic
        x = np.asarray(obs, dtype=np.float32)
        single = x.ndim == 1
        if single:
            x = x[None]
        per = L.OBS_DIM + (L.TRAFFIC_DIM - 1) * K
        if x.ndim != 2 or x.shape[1] == 0 or x.shape[1] % per:
            raise ValueError("obs must be [%d] or [n_envs, N * %d]%s, got %r" % (per, per, " (own words, then 7 words per traffic record)" if K else "",
                                                                                 np.shape(obs)))
        n_envs, N = x.shape[0], x.shape[1] // per
        rows = torch.from_numpy(np.ascontiguousarray(x[:, :N * L.OBS_DIM]).reshape(n_envs, N, L.OBS_DIM)).to(dev)
        tr = None
        if K:      # the 7-word records, padded to 8 with a word that is not read
            rec = np.zeros((n_envs, N, K, L.TRAFFIC_DIM), np.float32)
            rec[..., :L.TRAFFIC_DIM - 1] = x[:, N * L.OBS_DIM:].reshape(n_envs, N, K, L.TRAFFIC_DIM - 1)
            tr = torch.from_numpy(rec).to(dev)
        res = AtcVecEnv.policy_forward(self._host, self.weights, rows, traffic=tr, rows_per_decision=n_envs * N, seed=self.seed,
                                       decision0=self.decision, deterministic=bool(deterministic), outputs=("flown",))
        if not deterministic:
            self.decision = (self.decision + 1) & 0xffffffff
        a = res["flown"][0].reshape(n_envs, N * L.ACT_DIM).cpu().numpy()
        return (a[0] if single else a), None
