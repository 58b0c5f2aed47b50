"""AtcVecEnv — B envs x N aircraft of the AtcGym.step() path, all state in device tensors, stepped by libatcstep.so.

Build-own batched surface (the reference has only the single-env AtcGym, atc_gym.py:22-365, and reaches parallelism
through stable-baselines' SubprocVecEnv x8, learning/atc-gym-stable-baselines.py:76-78).  Method names follow the
stable-baselines VecEnv protocol (reset / step / get_attr / seed / close) so that a PPO loop can consume it directly;
tensors stay on the device.  `auto_reset=True` gives VecEnv semantics: a finished env restarts inside the step and the
returned observation is the RAW reset observation (quirk of atc_gym.py:351,365 that SubprocVecEnv workers expose too).
"""
import ctypes as C

import numpy as np

from . import layout as L
from . import lib as _lib
from . import policy


def auto_grid_cell(num_envs, num_aircraft):
    """Cell size [nm] of the MVA lookup grid for a batch, by its number of aircraft slots (envs x next_pow2(aircraft)):
        4 096 .. 131 072 slots   0.0625 nm   (65 536 x 1, 8 192 x 16)
        up to 262 144 slots      0.125 nm    (4 096 x 64; and the tiny batches below 4 096 slots, whose step is a launch latency)
        beyond                   0.25 nm     (65 536 x 16)
    A finer grid puts fewer aircraft into cells a border passes through — whose records are a second dependent L2 round trip
    for the wavefront holding such an aircraft, the longest chain of a step — which is what a small, latency-bound batch feels
    (round 4, split cells in place: 65 536 x 1 fused 3.04 / 3.35 / 3.71 / 4.33 us per step at 0.0625 / 0.125 / 0.25 / 0.5 nm, single
    steps 5.93 / 6.29 / 6.68 / 6.97; 8 192 x 16 fused 2.42 / 2.51 / 2.87 / 3.3); a large batch is bound by HBM or instruction issue
    and only pays for the bigger table (LOWW: 11.6 MB at 0.0625 nm — it lives in the Infinity Cache —, 3.2 MB at 0.125, 0.9 MB at
    0.25; 65 536 x 16: 17.7 us single steps at 0.125 against 17.6 at 0.25, 4 096 x 64 the same at every size).  The sector
    compiler takes 5 s for LOWW at 0.0625 nm (1.4 s at 0.125), once per process and sector.  Results do not depend on the cell
    size (the lookup is exact for any)."""
    w = 1
    while w < int(num_aircraft):
        w *= 2
    slots = int(num_envs) * w
    if 4096 <= slots <= 131072:
        return 0.0625
    return 0.125 if slots <= 262144 else 0.25


class AtcVecEnv:
    def __init__(self, num_envs, num_aircraft=1, sim_parameters=None, scenario=None, device=0, auto_reset=True,
                 spawn="auto", seed=0, grid_cell="auto", want_raw_obs=False, want_ac_reward=False, want_min_sep=False,
                 want_term_obs=False, timestep_limit=6000, sep_nm=3.0, sep_ft=1000.0, conflict_reward=-200.0,
                 host_mapped=False, keep_active=False, want_packet=False, check_held=False, lds_table=True, traffic=0):
        """host_mapped=True keeps state and outputs in pinned host memory mapped into the device (zero-copy): the kernels
        read / write it over the host link, every call ends with a stream synchronisation, and what is returned are CPU
        tensors.  Meant for tiny latency-bound batches (the single-env AtcGym); large batches belong in HBM.
        host_mapped="io" maps only what crosses the host link every step (actions in, results out); the state stays in HBM.
        want_packet=True (host_mapped, N == 1) adds atc_out_t.packet: the step result as self-validating 16-byte chunks that a
        host can poll in mapped memory instead of synchronising the stream (see `poll_packet`).
        keep_active=True is the reference's single-aircraft rule (ATC_M_KEEP_ACTIVE): an aircraft that reaches the corridor
        ends the episode and stays under control instead of being handed over.
        check_held=True (debugging aid) verifies the promise of step(..., held=True) — the actions equal those of the previous
        step — on every such call and raises if it is broken (costs a device comparison and a synchronisation per step).
        traffic=K (1 .. 8) adds the traffic observation (atc_observe_traffic, include/atc_step.h): `self.traffic`, [B, N, K, 8]
        float32 — for every aircraft its K nearest other aircraft under control, nearest first, as records (present, distance,
        ahead, right, altitude difference, relative velocity ahead / right, slot) in the observing aircraft's own frame, scaled
        like the observation when the sim parameters normalise.  reset(), observe(), step() and step_skip() then launch it after
        their own call on the same stream and info["traffic"] is that tensor: it describes the state the env is in NOW (after an
        auto-reset: the fresh spawn state, consistent with the raw reset observation the step returns).  traffic=0 (default): no
        such tensor, launch or key."""
        torch = _lib._torch_cuda()
        self.torch = torch
        self._check_held = bool(check_held)
        self._prev_actions = None
        self.host_mapped = bool(host_mapped)
        from envs.atc import model, scenarios
        self.sim_parameters = sim_parameters if sim_parameters is not None else model.SimParameters(1)
        self.scenario_obj = scenario if scenario is not None else scenarios.LOWW()
        if not 1 <= num_aircraft <= L.MAX_AIRCRAFT:
            raise ValueError("1 <= num_aircraft <= %d" % L.MAX_AIRCRAFT)
        self.B, self.N = int(num_envs), int(num_aircraft)
        self.traffic_k = int(traffic)
        if not 0 <= self.traffic_k <= L.TRAFFIC_MAX_K:
            raise ValueError("0 <= traffic <= %d" % L.TRAFFIC_MAX_K)
        self.num_envs = self.B
        if grid_cell == "auto":
            # the batch's preferred cell size, or the next coarser one the sector's blob can hold (a sector a few times LOWW's
            # size does not fit 2^24 words at 0.0625 nm): an explicitly requested size that does not fit raises SectorTooLarge
            from .scenario import SectorTooLarge
            want = auto_grid_cell(self.B, self.N)
            for grid_cell in [c for c in (0.0625, 0.125, 0.25, 0.5, 1.0, 2.0) if c >= want] + [None]:
                try:
                    self.compiled = scenarios.compile_scenario(self.scenario_obj, grid_cell=grid_cell)
                    break
                except SectorTooLarge:
                    if grid_cell is None:
                        raise
        else:
            self.compiled = scenarios.compile_scenario(self.scenario_obj, grid_cell=grid_cell)
        self.grid_cell = grid_cell
        # (one-aircraft envs: the sector's LDS-resident lookup table goes along — the multi-step launches of batches that fit one
        # workgroup per CU answer the MVA lookup from LDS, include/atc_step.h ABI 21; `lds_table=False` keeps it off, for A/B runs)
        # (... batches the LDSG launch can serve: whole workgroups of 256 one-aircraft envs — a single env never gets there)
        self.sector = _lib.Scenario(self.compiled, device, lds_table=(self.N == 1 and self.B % 256 == 0 and bool(lds_table)))
        self.device = self.sector.device
        n_entry = self.compiled.n_entry
        if n_entry < 1:
            raise ValueError("scenario has no entry point")
        if spawn == "auto":
            spawn = "random" if (self.N == 1 and n_entry > 1) else "lattice"
        if spawn not in ("random", "lattice"):
            raise ValueError("spawn must be 'auto', 'random' or 'lattice'")
        sp = self.sim_parameters
        self.params = _lib.make_params(dt=sp.timestep, shaping=sp.reward_shaping, normalize=sp.normalize_state,
                                       discrete=sp.discrete_action_space, auto_reset=auto_reset,
                                       random_entry=(spawn == "random"), seed=seed, timestep_limit=timestep_limit,
                                       sep_nm=sep_nm, sep_ft=sep_ft, conflict_reward=conflict_reward,
                                       keep_active=keep_active)
        self.timestep_limit = timestep_limit
        B, N, BN, dev = self.B, self.N, self.B * self.N, self.device
        if self.host_mapped:
            z = lambda shape, dt: torch.zeros(shape, dtype=dt).pin_memory()  # noqa: E731
        else:
            z = lambda shape, dt: torch.zeros(shape, dtype=dt, device=dev)  # noqa: E731
        # host_mapped="io": only what crosses the host link every step (actions in, results out) lives in mapped host memory;
        # the state stays in HBM, so the kernel's state loads and stores do not pay the link's round trip
        zs = (lambda shape, dt: torch.zeros(shape, dtype=dt, device=dev)) if host_mapped == "io" else z  # noqa: E731
        self._new_output = z
        self.frame_steps = None   # [B] uint8: steps each env took in the last step_skip (allocated by the first one)
        f32, i32 = torch.float32, torch.int32
        # persistent state (atc_state_t): packed records, see include/atc_step.h
        self.ac = zs((BN, L.AC_WORDS), i32)    # x, y (position-grid counts), phi (heading counts), v (speed counts, unsigned)
        self.alt = zs(BN, torch.float64)       # altitude [ft]: the reference's float64 (ABI 20)
        self.last_act = zs((BN, L.LA_WORDS), i32)   # last accepted targets: v counts, phi counts, altitude target (float64, words 2..3)
        self.env = zs((B, L.ENV_WORDS), i32)   # per-step env record
        self.stats = zs((B, L.STAT_WORDS), i32)  # per-episode env record
        self.pos_origin, self.pos_k = self.compiled.pos_origin, self.compiled.pos_k
        # named views into the records (live memory, usable for reads and in-place writes)
        self.h = self.alt
        self.phi_fix = self.ac[:, L.AC_PHI]    # heading counts (deg = 180 + phi_fix 2^-23); `phi` / `v` below are copies in units
        self.v_fix = self.ac[:, L.AC_V]        # speed counts (unsigned 32-bit in an int32 word, kt = v_fix 2^-23)
        self.timesteps = self.env[:, L.ENV_TIMESTEPS]
        self.actions_taken = self.env[:, L.ENV_ACTIONS_TAKEN]
        self.total_reward = self.env[:, L.ENV_TOTAL_REWARD:L.ENV_TOTAL_REWARD + 1].view(f32).squeeze(1)
        self.episodes = self.stats[:, L.STAT_EPISODES]
        self.ep_length = self.stats[:, L.STAT_EP_LENGTH]
        self.ep_return = self.stats[:, L.STAT_EP_RETURN:L.STAT_EP_RETURN + 1].view(f32).squeeze(1)
        self.win_bits = self.stats[:, L.STAT_WIN_BITS]
        self.ep_actions = self.stats[:, L.STAT_EP_ACTIONS]
        # per-step outputs (atc_out_t)
        self.obs = z((B, N * L.OBS_DIM), f32)
        self.raw_obs = z((B, N * L.OBS_DIM), f32) if want_raw_obs else None
        self.reward = z(B, f32)
        self.ac_reward = z((B, N), f32) if want_ac_reward else None
        self.done = z(B, torch.uint8)
        self.flags = z((B, N), torch.int16)
        self.min_sep = z(B, f32) if want_min_sep else None
        self.term_obs = z((B, N * L.OBS_DIM), f32) if want_term_obs else None
        if want_packet and not (self.host_mapped and N == 1):
            raise ValueError("want_packet needs host_mapped=True and num_aircraft=1")
        self.packet = z((B, L.PKT_CHUNKS, 4), i32) if want_packet else None
        self.traffic = z((B, N, self.traffic_k, L.TRAFFIC_DIM), f32) if self.traffic_k else None
        self._traffic_ptr = self._ptr(self.traffic)
        # exact heading counts / last heading target of aircraft whose 32-bit heading fields are saturated ("WIDE", ABI 19): the
        # reference's heading is unbounded (model.py:104-120).  Untouched while headings stay inside (-76, 436) deg.
        # (allocated after everything a step streams through, so that those tensors sit where they would without it)
        self.phi_wide = zs((BN, L.PHI_WIDE_WORDS), torch.float64)
        self._state = _lib.AtcState(*[self._ptr(getattr(self, n)) for n in _lib.STATE_FIELDS])
        # twin of `params` with ATC_M_ACTIONS_HELD set: what step(held=True) and the held launchers pass.  A persistent object,
        # refreshed by seed() / refresh_params(), so that pre-bound launchers see parameter changes like plain launches do
        self._params_held = type(self.params).from_buffer_copy(self.params)
        self._bind_outputs()
        self.refresh_params()
        self._lib = _lib.load()
        self.reset(first=True)

    # ------------------------------------------------------------------------------------------------ plumbing
    def pack_outputs(self):
        """Re-homes obs / raw_obs / reward / flags / done of a small env batch in ONE contiguous byte buffer (plus a pinned
        host mirror) so that a host-side caller (AtcGym) fetches a whole step result with a single device->host copy.
        Returns (device_bytes, host_bytes, layout) with layout[name] = (offset, nbytes); in host-mapped mode the two are
        the same pinned buffer and no copy is needed at all."""
        torch = self.torch
        assert self.raw_obs is not None
        B, N = self.B, self.N
        sizes = [("obs", B * N * L.OBS_DIM * 4), ("raw_obs", B * N * L.OBS_DIM * 4), ("reward", B * 4),
                 ("flags", B * N * 2), ("done", B)]
        layout, off = {}, 0
        for name, nb in sizes:
            layout[name] = (off, nb)
            off += (nb + 15) & ~15
        host = torch.zeros(off, dtype=torch.uint8).pin_memory()
        dev = host if self.host_mapped else torch.zeros(off, dtype=torch.uint8, device=self.device)
        view = lambda name, dt, shape: dev[layout[name][0]:layout[name][0] + layout[name][1]].view(dt).view(shape)  # noqa: E731
        self.obs = view("obs", torch.float32, (B, N * L.OBS_DIM))
        self.raw_obs = view("raw_obs", torch.float32, (B, N * L.OBS_DIM))
        self.reward = view("reward", torch.float32, (B,))
        self.flags = view("flags", torch.int16, (B, N))
        self.done = view("done", torch.uint8, (B,))
        self._bind_outputs()
        return dev, host, layout

    def _ptr(self, t):
        """Device address of a tensor this env hands to the library (mapped address for pinned host tensors)."""
        if t is None:
            return None
        return t.data_ptr() if t.is_cuda else _lib.mapped_ptr(t)

    def _make_out(self, *tensors):
        return _lib.AtcOut(*[self._ptr(t) for t in tensors])

    def _bind_outputs(self):
        """(Re)builds atc_out_t for this env's own output tensors and everything step() reuses from call to call."""
        self._out = self._make_out(self.obs, self.raw_obs, self.reward, self.ac_reward, self.done, self.flags,
                                   self.min_sep, self.term_obs, getattr(self, "packet", None))
        self._out_ref = C.byref(self._out)
        self._state_ref = C.byref(self._state)
        self._params_ref = C.byref(self.params)
        self._params_held_ref = C.byref(self._params_held)
        self._n_act = self.B * self.N * L.ACT_DIM
        self._info_cache = self._info()
        self._info_skip = None

    def _bind_frame_steps(self):
        """What step_skip() and branch(into=self) need on their first call (and again after _bind_outputs): frame_steps, [B] uint8, allocated
        once, and the info dict that carries it.  _info_skip is not None only behind this."""
        if self.frame_steps is None:
            self.frame_steps = self._new_output(self.B, self.torch.uint8)
            self._frame_steps_ptr = self._ptr(self.frame_steps)
        self._info_skip = dict(self._info_cache, frame_steps=self.frame_steps)

    def _finish(self):
        if self.host_mapped:  # results live in host memory: valid only once the stream has drained
            self.torch.cuda.current_stream(self.device).synchronize()

    def _stream(self):
        return _lib.current_stream_ptr(self.device)

    @property
    def action_dim(self):
        return self.N * L.ACT_DIM

    @property
    def obs_dim(self):
        return self.N * L.OBS_DIM

    # ------------------------------------------------------------------------------------------------ VecEnv surface
    def seed(self, seed=None):
        self.params.seed = int(seed or 0) & (2 ** 64 - 1)
        self.refresh_params()
        return [seed] * self.B

    def refresh_params(self):
        """Copies `params` into its held-action twin (the struct launches with ATC_M_ACTIONS_HELD pass).  seed() calls it; call
        it after changing a field of `env.params` directly, or launchers made with held=True keep the old value."""
        C.memmove(C.byref(self._params_held), C.byref(self.params), C.sizeof(self.params))
        self._params_held.mode |= L.M_ACTIONS_HELD

    def _as_mask(self, mask):
        """An env mask (None: every env) as the contiguous uint8 device tensor atc_reset / atc_observe read"""
        return None if mask is None else self.torch.as_tensor(mask, device=self.device).to(self.torch.uint8).contiguous()

    def reset(self, mask=None, first=False):
        """AtcGym.reset (atc_gym.py:337-365) for all envs (or those with mask != 0); returns RAW obs [B, N*10]."""
        m = self._as_mask(mask)
        with self.torch.cuda.device(self.device):
            _lib.check(self._lib.atc_reset(self.sector.handle, self.B, self.N, C.byref(self._state),
                                           self._ptr(m), self._ptr(self.obs),
                                           C.byref(self.params), int(first), self._stream()))
            self._launch_traffic()
        self._finish()
        return self.obs

    def observe(self, mask=None):
        """Raw observation (mva = 0) of the current state, like the tail of AtcGym.reset (atc_gym.py:351,365)."""
        m = self._as_mask(mask)
        with self.torch.cuda.device(self.device):
            _lib.check(self._lib.atc_observe(self.sector.handle, self.B, self.N, C.byref(self._state),
                                             self._ptr(m), self._ptr(self.obs),
                                             C.byref(self.params), self._stream()))
            self._launch_traffic()
        self._finish()
        return self.obs

    def _launch_traffic(self):
        """atc_observe_traffic of the current state into self.traffic, on the current stream (nothing with traffic=0)"""
        if self.traffic_k:
            rc = self._lib.atc_observe_traffic(self.sector.handle, self.B, self.N, self.traffic_k, self._state_ref, self._traffic_ptr,
                                               self._params_ref, self.torch.cuda.current_stream().cuda_stream)
            if rc:
                _lib.check(rc)

    def observe_traffic(self):
        """The traffic observation of the CURRENT state (atc_observe_traffic): launches on the current stream and returns
        self.traffic, [B, N, K, 8] — see the class's `traffic` argument.  Needs AtcVecEnv(traffic=K) with K >= 1."""
        if not self.traffic_k:
            raise ValueError("this env was made without a traffic observation: AtcVecEnv(..., traffic=K), 1 <= K <= %d" % L.TRAFFIC_MAX_K)
        with self.torch.cuda.device(self.device):
            self._launch_traffic()
        self._finish()
        return self.traffic

    def _as_actions(self, actions, lead=()):
        torch = self.torch
        a = actions if torch.is_tensor(actions) else torch.as_tensor(np.asarray(actions, dtype=np.float32))
        if not (self.host_mapped and not a.is_cuda and a.is_pinned() and a.dtype == torch.float32):
            a = a.to(device=self.device, dtype=torch.float32)
        a = a.contiguous()
        want = int(np.prod(lead, dtype=np.int64)) * self.B * self.N * L.ACT_DIM if lead else self.B * self.N * L.ACT_DIM
        if a.numel() != want:
            raise ValueError("actions must have %d elements, got %d" % (want, a.numel()))
        return a

    def step(self, actions, held=False):
        """AtcGym.step (atc_gym.py:128-192) for every env.  actions: [B, N, 3] (or [B, N*3]) float tensor / array:
        continuous in [-1, 1] or discrete indices (atc_gym.py:318-335).  Returns (obs [B,N*10], reward [B], done [B]
        uint8, info) — device tensors that are overwritten by the next step.
        held=True is the caller's promise that `actions` holds the same values as in the previous step of these envs (a
        held action block / frame skip, learning/atc-gym-demo.py:18-19; ATC_M_ACTIONS_HELD): same results, and the kernel
        skips the last-action record."""
        if self._check_held:
            cur = self._as_actions(actions).reshape(-1).to("cpu", copy=True)
            if held and (self._prev_actions is None or not self.torch.equal(cur.view(self.torch.int32),
                                                                              self._prev_actions.view(self.torch.int32))):
                raise ValueError("step(held=True): the actions differ from the previous step's (or there was none)")
            self._prev_actions = cur
        torch = self.torch
        pref = self._params_held_ref if held else self._params_ref
        # fast path: a float32 device tensor of the right size on this env's (current) device is handed over as it is —
        # small batches are host-bound otherwise (8 192 x 16: 6.4 us on the GPU against 10.4 us of Python per call)
        if (torch.is_tensor(actions) and actions.is_cuda and actions.dtype is torch.float32 and actions.is_contiguous()
                and actions.numel() == self._n_act and actions.device == self.device
                and torch.cuda.current_device() == self.device.index and not self.host_mapped):
            rc = self._lib.atc_step(self.sector.handle, self.B, self.N, self._state_ref, actions.data_ptr(), self._out_ref,
                                    pref, torch.cuda.current_stream().cuda_stream)
            if rc:
                _lib.check(rc)
            if self.traffic_k:
                self._launch_traffic()
            self._keep = actions
            return self.obs, self.reward, self.done, self._info_cache
        a = self._as_actions(actions)
        with torch.cuda.device(self.device):
            _lib.check(self._lib.atc_step(self.sector.handle, self.B, self.N, C.byref(self._state), self._ptr(a),
                                          C.byref(self._out), pref, self._stream()))
            self._launch_traffic()
        self._keep = a
        self._finish()
        return self.obs, self.reward, self.done, self._info_cache

    def step_skip(self, actions, skip):
        """Frame skip (atc_step_skip; the reference's demo loop, learning/atc-gym-demo.py:14-22): every env repeats `actions` until
        it reports done or has taken `skip` steps (1 .. 255) — ONE launch, one transition per env.  Returns (obs, reward, done,
        info) in this env's own output tensors like step(): the observation after the env's last executed step, the float32 sum
        of the executed steps' rewards (in step order), done if the episode ended inside the block; info["flags"] is the OR of the
        executed steps' flag words, info["frame_steps"] the [B] uint8 tensor of executed steps.  An env that ends early is not
        stepped again in the call (with auto_reset it waits in its fresh spawn state), so a transition never spans two episodes.
        Bit for bit what a host loop over step() computes; step_skip(a, 1) is step(a)."""
        torch = self.torch
        skip = int(skip)
        if not 1 <= skip <= L.SKIP_MAX:
            raise ValueError("1 <= skip <= %d" % L.SKIP_MAX)
        if self._info_skip is None:
            self._bind_frame_steps()
        self._prev_actions = None   # (check_held: the block's last step is not a step() call to repeat)
        if (torch.is_tensor(actions) and actions.is_cuda and actions.dtype is torch.float32 and actions.is_contiguous()
                and actions.numel() == self._n_act and actions.device == self.device
                and torch.cuda.current_device() == self.device.index and not self.host_mapped):
            rc = self._lib.atc_step_skip(self.sector.handle, self.B, self.N, skip, self._state_ref, actions.data_ptr(), self._out_ref,
                                         self._frame_steps_ptr, self._params_ref, torch.cuda.current_stream().cuda_stream)
            if rc:
                _lib.check(rc)
            if self.traffic_k:
                self._launch_traffic()
            self._keep = actions
            return self.obs, self.reward, self.done, self._info_skip
        a = self._as_actions(actions)
        with torch.cuda.device(self.device):
            _lib.check(self._lib.atc_step_skip(self.sector.handle, self.B, self.N, skip, C.byref(self._state), self._ptr(a),
                                               C.byref(self._out), self._frame_steps_ptr, C.byref(self.params), self._stream()))
            self._launch_traffic()
        self._keep = a
        self._finish()
        return self.obs, self.reward, self.done, self._info_skip

    LOOKAHEAD_OUTPUTS = ("flags", "min_sep", "ac_reward", "obs")

    def lookahead(self, actions, K, outputs=("flags", "min_sep")):
        """What-if query (atc_lookahead, include/atc_step.h): for each of M candidate decisions per env, what step_skip(actions[m], K)
        would return from the state the env is in NOW — in one launch that writes no state.  actions: [M, B, N, 3] (or [M, B, N*3]),
        1 <= M <= 64, 1 <= K <= 255.  Returns a dict of device tensors: reward [M, B] float32, done [M, B] uint8, n_steps [M, B]
        uint8 always, and each of flags [M, B, N] int16, min_sep [M, B], ac_reward [M, B, N], obs [M, B, N*10] that `outputs`
        names (none of them: the kernel's fast form).  The tensors are allocated once per (M, outputs) and overwritten by the next
        such call.  Runs on the current stream; env.obs / env.traffic, every bound step output and the whole env state — episode
        records included — are left as they are.  An env-candidate with a WIDE heading (an out-of-range heading action or state) is
        not evaluated: n_steps == 0 and zeros.  AtcSBVecEnv and AtcGym deliberately have no such method."""
        return self._score_candidates(actions, K, outputs, plan=False)

    PLAN_OUTPUTS = ("seg_reward", "flags", "min_sep", "ac_reward", "obs")

    def lookahead_plan(self, actions, K, outputs=("seg_reward", "flags", "min_sep")):
        """Plan query (atc_lookahead_plan, include/atc_step.h): lookahead() for candidates that are sequences.  actions:
        [M, H, B, N, 3] (or [M, H, B, N*3]) — M plans per env, each H decisions held for K steps one after the other, 1 <= M <= 64,
        1 <= H <= 16, 1 <= K <= 255.  For each plan: what chaining step_skip(actions[m, h], K) over h would return from the state the
        env is in NOW, stopping at the env's first done — in one launch that writes no state.  Returns a dict of device tensors:
        reward [M, B] float32 (the sum of the executed segments' rewards, in segment order), done [M, B] uint8, n_steps [M, B] int16
        (executed steps in total) always, and each of seg_reward [M, H, B] (per-segment rewards, 0 behind the stop: weight them by a
        discount in torch), flags [M, B, N] int16, min_sep [M, B], ac_reward [M, B, N], obs [M, B, N*10] that `outputs` names
        (none of the last four: the kernel's fast form).  The tensors are allocated once per (M, H, outputs) and overwritten by the
        next such call.  Runs on the current stream; env.obs / env.traffic, every bound step output and the whole env state are left
        as they are.  An env-candidate with a WIDE heading is not evaluated: n_steps == 0 and zeros.  H == 1 is lookahead()."""
        return self._score_candidates(actions, K, outputs, plan=True)

    def _score_candidates(self, actions, K, outputs, plan):
        """lookahead() (plan=False: actions [M, ...]) and lookahead_plan() (plan=True: actions [M, H, ...]): the argument checks in
        their order, the result tensors and output struct cached per (M[, H], outputs), the launch"""
        torch = self.torch
        K = self._held_k(K)
        if plan and (not hasattr(actions, "shape") or len(actions.shape) < 2):
            raise ValueError("actions must be [M, H, B, N, 3] or [M, H, B, N*3]")
        M = int(actions.shape[0]) if hasattr(actions, "shape") else len(actions)
        if not 1 <= M <= L.LOOKAHEAD_MAX_M:
            raise ValueError("1 <= M (actions.shape[0]) <= %d" % L.LOOKAHEAD_MAX_M)
        lead = (M, int(actions.shape[1])) if plan else (M,)
        if plan and not 1 <= lead[1] <= L.PLAN_MAX_H:
            raise ValueError("1 <= H (actions.shape[1]) <= %d" % L.PLAN_MAX_H)
        allowed = self.PLAN_OUTPUTS if plan else self.LOOKAHEAD_OUTPUTS
        if not set(outputs) <= set(allowed):
            raise ValueError("outputs must be a subset of %r" % (allowed,))
        outputs = tuple(n for n in allowed if n in outputs)
        a = self._as_actions(actions, lead=lead)
        res, out = self._candidate_results("_plan_cache" if plan else "_lookahead_cache", lead, outputs, plan)
        call = self._lib.atc_lookahead_plan if plan else self._lib.atc_lookahead
        with torch.cuda.device(self.device):   # (the C argument order: K, [H,] M)
            _lib.check(call(self.sector.handle, self.B, self.N, K, *lead[::-1], C.byref(self._state), self._ptr(a), C.byref(out),
                            C.byref(self.params), self._stream()))
        setattr(self, "_keep_plan" if plan else "_keep_lookahead", a)   # the actions outlive the launch, one tensor per call kind
        self._finish()
        return res

    def _candidate_results(self, cache_name, lead, outputs, plan, struct=None):
        """The result tensors of a candidate-scoring call and the output struct that points at them, made once per (M[, H], outputs).
        struct: (ctypes type, field names) of a call whose output struct is neither atc_plan_out_t nor atc_lookahead_out_t"""
        torch = self.torch
        cache = self.__dict__.setdefault(cache_name, {})
        key = lead + (outputs,)
        if key not in cache:
            M, B, N, z = lead[0], self.B, self.N, self._new_output
            shapes = {"reward": ((M, B), torch.float32), "done": ((M, B), torch.uint8), "n_steps": ((M, B), torch.int16 if plan else torch.uint8),
                      "seg_reward": (lead + (B,), torch.float32), "flags": ((M, B, N), torch.int16), "min_sep": ((M, B), torch.float32),
                      "ac_reward": ((M, B, N), torch.float32), "obs": ((M, B, N * L.OBS_DIM), torch.float32),
                      "flown": (lead + (B, N, L.ACT_DIM), torch.float32), "logp": (lead + (B, N), torch.float32)}
            res = {n: z(*shapes[n]) for n in ("reward", "done", "n_steps") + outputs}
            out_type, fields = struct or ((_lib.AtcPlanOut, _lib.PLAN_FIELDS) if plan else (_lib.AtcLookaheadOut, _lib.LOOKAHEAD_FIELDS))
            cache[key] = (res, out_type(*[self._ptr(res.get(n)) for n in fields]))
        return cache[key]

    @staticmethod
    def _held_k(K):
        """K of the candidate calls (the steps a decision is held for) as an int; outside 1 .. 255: ValueError"""
        K = int(K)
        if not 1 <= K <= L.SKIP_MAX:
            raise ValueError("1 <= K <= %d" % L.SKIP_MAX)
        return K

    def _draw_h(self, mean):
        """H of the drawn-plan calls: mean is [H, B, N, 3] or [H, B, N*3]; outside 1 .. 16: ValueError"""
        if not hasattr(mean, "shape") or len(mean.shape) < 2:
            raise ValueError("mean must be [H, B, N, 3] or [H, B, N*3]")
        H = int(mean.shape[0])
        if not 1 <= H <= L.PLAN_MAX_H:
            raise ValueError("1 <= H (mean.shape[0]) <= %d" % L.PLAN_MAX_H)
        return H

    @staticmethod
    def _drawn_m(M, name="M"):
        """M of the drawn-plan calls as an int; outside 1 .. 1024: ValueError"""
        M = int(M)
        if not 1 <= M <= L.SAMPLE_MAX_M:
            raise ValueError("1 <= %s <= %d" % (name, L.SAMPLE_MAX_M))
        return M

    def _refuse_discrete(self):
        if self.params.mode & L.M_DISCRETE:
            raise ValueError("only the continuous action space is drawn (this env has discrete actions)")

    def _as_tensor(self, v):
        return v if self.torch.is_tensor(v) else self.torch.as_tensor(np.asarray(v))

    def _as_index(self, index, shape, n):
        """An integer tensor as the contiguous int32 device tensor of `shape` the library reads: -1 where the value is outside 0 .. n-1
        (the range test on the caller's own dtype: an int64 value beyond 32 bits must be refused, not wrapped into range)"""
        index = index.to(device=self.device).reshape(shape)
        return self.torch.where((index >= 0) & (index < n), index, self.torch.full_like(index, -1)).to(self.torch.int32).contiguous()

    def _to_device(self, mu, sd):
        """mean and std for a call that takes device tensors only: a host-mapped env's pinned pair is copied to the device"""
        if self.host_mapped and not (mu.is_cuda and sd.is_cuda):
            return mu.to(self.device), sd.to(self.device)
        return mu, sd

    def _on_device(self, t, dtypes, shape, what=None, text=None, elements=False):
        """`t` if it is a contiguous tensor of one of `dtypes` on this env's device and, where `shape` is given, of that shape (elements=True:
        of that many elements); ValueError otherwise — `text % (shape, device)` in the caller's words, or in terms of `what`"""
        torch = self.torch
        if not (torch.is_tensor(t) and t.device == self.device and t.dtype in dtypes and t.is_contiguous()
                and (shape is None or (t.numel() == int(np.prod(shape, dtype=np.int64)) if elements else t.shape == shape))):
            raise ValueError(text % (shape, self.device) if text else "%s must be a contiguous %s tensor%s on %s" % (
                what, " / ".join(str(d) for d in dtypes), "" if shape is None else " of %r" % (shape,), self.device))
        return t

    def _results(self, out, want, required, refusal=None, others=False):
        """The result tensors of a call with an out= dict.  want: {name: (dtypes, shape)}.  Without `out`: fresh tensors of every name.  With
        it: out's own — every `required` name there and, unless `others`, none that `want` does not know (ValueError otherwise: `refusal`,
        or "out must be a dict with" want's names), each checked by _on_device as "out['name']" — and nothing is allocated."""
        if out is None:
            return {n: self.torch.empty(shape, dtype=dt[0], device=self.device) for n, (dt, shape) in want.items()}
        if not isinstance(out, dict) or not required <= out.keys() or not (others or out.keys() <= want.keys()):
            raise ValueError(refusal or "out must be a dict with %s" % ", ".join(want))
        return {n: AtcVecEnv._on_device(self, out[n], dt, shape, "out[%r]" % n) for n, (dt, shape) in want.items() if n in out}

    def _draw_source(self, H, mean, std, seed, iteration, mean_first):
        """(mean, std, atc_plan_draw_t) as the library reads them: contiguous float32 tensors of H * B * N * 3 elements (a python float
        for std is broadcast once into a cached tensor)"""
        torch = self.torch
        mu = self._as_actions(mean, lead=(H,))
        if isinstance(std, (int, float)):
            cache = self.__dict__.setdefault("_std_cache", {})
            key = (H, float(std))
            if key not in cache:
                cache.clear()   # (one broadcast tensor at a time: a planner keeps its value from call to call)
                cache[key] = torch.full((H, self.B, self.N * L.ACT_DIM), float(std), dtype=torch.float32, device=mu.device,
                                        pin_memory=not mu.is_cuda)
            sd = cache[key]
        else:
            sd = self._as_actions(std, lead=(H,))
        if not 0 <= int(iteration) < 2 ** 32:
            raise ValueError("0 <= iteration < 2**32")
        dr = _lib.AtcPlanDraw(int(seed) & (2 ** 64 - 1), int(iteration), L.DRAW_MEAN_FIRST if mean_first else 0)
        return mu, sd, dr

    def lookahead_plan_sampled(self, mean, std, K, M, seed=0, iteration=0, mean_first=True, outputs=("seg_reward",)):
        """Plan query with the candidates DRAWN inside the launch (atc_lookahead_plan_sampled, include/atc_step.h): lookahead_plan() on
        the M plans draw_plans(mean, std, M, seed, iteration, mean_first) would return, bit for bit, without that [M, H, B, N, 3]
        tensor ever existing — so M goes up to 1024.  mean, std: [H, B, N, 3] (or [H, B, N*3]) float tensors, std also a python
        float (broadcast once into a cached tensor); every action component is clamp(mean + std * z, -1, 1) with z a function of (seed,
        iteration, m, h, aircraft, component) alone, mean 0 and variance 1.  mean_first: candidate 0 is the (clamped) mean itself.
        1 <= K <= 255, 1 <= H <= 16, 1 <= M <= 1024; continuous action space only.  Returns lookahead_plan()'s dict; the tensors are
        allocated once per (M, H, outputs) and overwritten by the next such call.  The env state is left as it is.  Regenerate the few
        plans you need (elites, the winner) with draw_plans(index=...).  AtcSBVecEnv and AtcGym deliberately have no such method."""
        torch = self.torch
        K = self._held_k(K)
        H = self._draw_h(mean)
        M = self._drawn_m(M)
        mu, sd, dr = self._draw_source(H, mean, std, seed, iteration, mean_first)
        if not set(outputs) <= set(self.PLAN_OUTPUTS):
            raise ValueError("outputs must be a subset of %r" % (self.PLAN_OUTPUTS,))
        outputs = tuple(n for n in self.PLAN_OUTPUTS if n in outputs)
        self._refuse_discrete()
        res, out = self._candidate_results("_plan_sampled_cache", (M, H), outputs, True)
        with torch.cuda.device(self.device):
            _lib.check(self._lib.atc_lookahead_plan_sampled(self.sector.handle, self.B, self.N, K, H, M, C.byref(self._state), self._ptr(mu),
                                                            self._ptr(sd), C.byref(dr), C.byref(out), C.byref(self.params), self._stream()))
        self._keep_plan_sampled = (mu, sd)   # mean and std outlive the launch (one pair per call kind, like _keep_plan)
        self._finish()
        return res

    LOOKAHEAD_POLICY_OUTPUTS = PLAN_OUTPUTS + ("flown", "logp")

    def lookahead_policy(self, weights, K, H, *, first=None, M=None, seed=0, decision0=0, deterministic=False, obs0=None,
                         outputs=("flags", "min_sep"), out=None):
        """Plan query whose candidates are CONTINUED BY THE POLICY inside the launch (atc_lookahead_policy, include/atc_step.h): M candidates
        per env flown on copies of the state the env is in NOW for H segments of K steps, each stopping at its first done — in one launch
        that writes no state and no per-step stream.  weights: the POLICY_WORDS-word tensor of atc_hip.policy.pack_mlp (a traffic policy is
        refused).  first: [M, B, N, 3] (or [M, B, N*3]) clamped actions as lookahead() takes them — segment 0 flies first[m] and the policy
        decides segments 1 .. H-1 from the observation the candidate is then in ("if I take this decision and then go on as I would");
        without it M is given and the policy decides every segment, segment 0 from obs0 (default: the env's bound observation tensor).
        The decisions use rollout_policy's key with decision0, decision0 + 1, ... and the aircraft numbering of branch()'s child batch, so
        the call equals select() / branch() into a child, rollout_policy(hold=K) on it and a fold of its [T, M*B] arrays.  1 <= K <= 255,
        1 <= H <= 16, 1 <= M <= 1024; continuous action space only.
        Returns lookahead_plan()'s dict — reward, done [M, B], n_steps [M, B] int16 and seg_reward [M, H, B] always; flags, min_sep,
        ac_reward, obs as `outputs` names them — plus, where named, flown [M, H, B, N, 3] (the clamped action each segment flew; rows of
        segments an env did not run are left alone; flown[:, 0] is what step_skip takes to execute a winner) and logp [M, H, B, N]
        (the segments the policy decided).  Without `out` the tensors are allocated once per (M, H, outputs) and overwritten by the next
        such call; out: a dict of preallocated tensors of those names (reward and done at least) — its keys are the outputs, and nothing
        is allocated.  The env state is left as it is."""
        torch = self.torch
        K = AtcVecEnv._held_k(K)
        H = int(H)
        if not 1 <= H <= L.PLAN_MAX_H:
            raise ValueError("1 <= H <= %d" % L.PLAN_MAX_H)
        if not torch.is_tensor(weights):
            raise ValueError("weights must be the packed float32 tensor of atc_hip.policy.pack_mlp")
        if policy.traffic_of(weights.numel()) != 0:
            raise ValueError("lookahead_policy takes the ten-word policy only: these weights are a policy that sees traffic, which is out of its scope")
        w = AtcVecEnv._on_device(self, weights, (torch.float32,), (L.POLICY_WORDS,),
                                 text="weights must be the contiguous float32 tensor of %r words (atc_hip.policy.pack_mlp) on %s", elements=True)
        AtcVecEnv._refuse_discrete(self)
        B, N = self.B, self.N
        if first is not None:
            if not hasattr(first, "shape") or len(first.shape) < 2:
                raise ValueError("first must be [M, B, N, 3] or [M, B, N*3]")
            if M is not None and int(M) != int(first.shape[0]):
                raise ValueError("M is first.shape[0] where first is given")
            M = AtcVecEnv._drawn_m(int(first.shape[0]), "M (first.shape[0])")
            a, x0 = AtcVecEnv._as_actions(self, first, lead=(M,)), None
        else:
            if M is None:
                raise ValueError("M is required where first is not given")
            M = AtcVecEnv._drawn_m(M)
            a, x0 = None, self.obs if obs0 is None else obs0
            if not (torch.is_tensor(x0) and x0.dtype == torch.float32 and x0.is_contiguous() and x0.numel() == B * N * L.OBS_DIM):
                raise ValueError("obs0 must be a contiguous float32 tensor of B*N*%d words" % L.OBS_DIM)
        if M * B * N >= 2 ** 32:
            raise ValueError("M * B * N must stay below 2**32")
        if out is None:
            if not set(outputs) <= set(AtcVecEnv.LOOKAHEAD_POLICY_OUTPUTS):
                raise ValueError("outputs must be a subset of %r" % (AtcVecEnv.LOOKAHEAD_POLICY_OUTPUTS,))
            names = tuple(n for n in AtcVecEnv.LOOKAHEAD_POLICY_OUTPUTS if n in outputs or n == "seg_reward")
            res, o = AtcVecEnv._candidate_results(self, "_lookahead_policy_cache", (M, H), names, True, (_lib.AtcLookaheadPolicyOut, _lib.LOOKAHEAD_POLICY_FIELDS))
        else:
            f32, i16 = (torch.float32,), (torch.int16, getattr(torch, "uint16", torch.int16))
            want = {"reward": (f32, (M, B)), "done": ((torch.uint8,), (M, B)), "n_steps": (i16, (M, B)), "seg_reward": (f32, (M, H, B)),
                    "flags": (i16, (M, B, N)), "ac_reward": (f32, (M, B, N)), "min_sep": (f32, (M, B)), "obs": (f32, (M, B, N * L.OBS_DIM)),
                    "flown": (f32, (M, H, B, N, L.ACT_DIM)), "logp": (f32, (M, H, B, N))}
            res = AtcVecEnv._results(self, out, want, {"reward", "done"}, "out must be a dict with reward, done and any of %s" % ", ".join(want))
            o = _lib.AtcLookaheadPolicyOut(*[res[n].data_ptr() if n in res else None for n in _lib.LOOKAHEAD_POLICY_FIELDS])
        pol = _lib.AtcPolicy(w.data_ptr(), L.POLICY_HIDDEN, L.POLICY_DETERMINISTIC if deterministic else 0, int(seed) & (2 ** 64 - 1),
                             int(decision0) & 0xffffffff, 0)
        fn = self._lib.atc_lookahead_policy
        with torch.cuda.device(self.device):
            rc = fn(self.sector.handle, B, N, K, H, M, C.byref(self._state), None if x0 is None else self._ptr(x0),
                                                None if a is None else self._ptr(a), C.byref(pol), C.byref(o), C.byref(self.params), self._stream())
            if rc:
                _lib.check(rc)
        self._keep_lookahead_policy = (w, x0, a)   # the inputs outlive the launch (one set per call kind, like _keep_plan)
        if self.host_mapped:
            self._finish()
        return res

    def draw_plans(self, mean, std, M, seed=0, iteration=0, mean_first=True, index=None, out=None):
        """The plans lookahead_plan_sampled() scores, as a tensor (atc_plan_draw, include/atc_step.h).  Without `index`: all M
        candidates, [M, H, B, N, 3].  With `index` ([E, B] or [B], any integer dtype): [E, H, B, N, 3] whose row r holds, for env e,
        candidate index[r, e] — the elites of a CEM iteration, the winner; an env whose index is outside 0 .. M-1 keeps what the row
        holds (zeros in a fresh tensor; a value beyond 32 bits is out of range, never wrapped).  out: a float32 device tensor of
        that many elements to write into instead of a fresh one.  mean, std, M, seed, iteration, mean_first: as in
        lookahead_plan_sampled()."""
        torch = self.torch
        H = self._draw_h(mean)
        M = self._drawn_m(M)
        idx, R = None, M
        if index is not None:
            index = self._as_tensor(index)
            if index.dtype.is_floating_point or index.dtype is torch.bool or index.numel() < 1 or index.numel() % self.B:
                raise ValueError("index must be an integer tensor [E, B] or [B] (B = %d)" % self.B)
            R = index.numel() // self.B
            idx = self._as_index(index, (R, self.B), M)
        mu, sd, dr = self._draw_source(H, mean, std, seed, iteration, mean_first)
        self._refuse_discrete()
        shape = (R, H, self.B, self.N, L.ACT_DIM)
        if out is None:
            out = (torch.empty if idx is None else torch.zeros)(shape, dtype=torch.float32, device=self.device)
        else:
            self._on_device(out, (torch.float32,), shape, text="out must be a contiguous float32 tensor of %s on %s", elements=True)
        mu, sd = self._to_device(mu, sd)
        with torch.cuda.device(self.device):
            _lib.check(self._lib.atc_plan_draw(self.sector.handle, self.B, self.N, H, M, self._ptr(mu), self._ptr(sd), C.byref(dr),
                                               None if idx is None else idx.data_ptr(), R, out.data_ptr(), C.byref(self.params), self._stream()))
        self._keep_draw = (mu, sd, idx)
        return out.view(shape)

    def refit_plans(self, mean, std, M, weight, seed=0, iteration=0, mean_first=True, out=None, std_min=0.0):
        """The distribution update of a sampling planner on the plans lookahead_plan_sampled() scored, none materialised
        (atc_plan_refit, include/atc_step.h): the weighted mean and standard deviation over the M candidates of (seed, iteration), each
        regenerated inside the launch.  weight: [M, B] (converted to contiguous float32 on this env's device) — 0/1 for CEM elites,
        softmax(score / temperature) for MPPI; a candidate takes part in its env iff 0 < weight <= FLT_MAX (NaN, zero, negative and
        infinite weights leave it out; give 0 to candidates with n_steps == 0).  Returns (mean', std'), each [H, B, N, 3]: without
        `out`, fresh tensors that start as copies of the inputs as the library reads them, so an env with no participating candidate
        keeps its distribution; out=(mean_t, std_t) names contiguous float32 device tensors of H*B*N*3 elements to write instead — they
        may be the inputs themselves (an in-place update), any other overlap is refused by the library.  std_min > 0 clamps the
        returned std from below (torch, on the small result).  mean, std, M, seed, iteration, mean_first: as in
        lookahead_plan_sampled(); continuous action space only."""
        torch = self.torch
        H = self._draw_h(mean)
        M = self._drawn_m(M)
        weight = self._as_tensor(weight)
        if tuple(weight.shape) != (M, self.B):
            raise ValueError("weight must be [M, B] = [%d, %d], got %r" % (M, self.B, tuple(weight.shape)))
        w = weight.to(device=self.device, dtype=torch.float32).contiguous()
        mu, sd, dr = self._draw_source(H, mean, std, seed, iteration, mean_first)
        self._refuse_discrete()
        mu, sd = self._to_device(mu, sd)
        shape = (H, self.B, self.N, L.ACT_DIM)
        if out is None:
            new_mu, new_sd = mu.clone(), sd.clone()
        else:
            if not (isinstance(out, (tuple, list)) and len(out) == 2):
                raise ValueError("out must be a pair (mean_t, std_t)")
            new_mu, new_sd = out
            for t in (new_mu, new_sd):
                self._on_device(t, (torch.float32,), shape, text="out must hold contiguous float32 tensors of %s on %s", elements=True)
        with torch.cuda.device(self.device):
            _lib.check(self._lib.atc_plan_refit(self.sector.handle, self.B, self.N, H, M, self._ptr(mu), self._ptr(sd), C.byref(dr),
                                                w.data_ptr(), new_mu.data_ptr(), new_sd.data_ptr(), C.byref(self.params), self._stream()))
        self._keep_refit = (mu, sd, w)   # the inputs outlive the launch (like _keep_draw)
        if float(std_min) > 0.0:
            new_sd.clamp_(min=float(std_min))
        return new_mu.view(shape), new_sd.view(shape)

    def score_plans(self, seg_reward, n_steps=None, *, mode="elite", elites=None, temperature=None, gamma=1.0, top=1, out=None):
        """What lies between lookahead_plan_sampled() and refit_plans() in a sampling planner's iteration, in one launch on this env's
        current stream (atc_plan_score, include/atc_step.h).  seg_reward: [M, H, B] float32 and n_steps: [M, B] int16 / uint16 or None,
        contiguous tensors on this env's device as lookahead_plan_sampled() returns them (nothing is converted: ValueError otherwise).
        score[m, e] = seg[m, 0, e] + seg[m, 1, e] * gamma + seg[m, 2, e] * (gamma * gamma) + ... in fp32, left to right, the discount a
        running product.  A candidate is VALID iff it was evaluated (n_steps != 0, or n_steps is None) and its score is finite; the
        valid candidates of an env are ordered by score descending, equal scores (+0 == -0) to the LOWER candidate number.
        mode="elite": weight 1.0 for the first min(elites, valid) of that order, 0.0 for the rest (1 <= elites <= M).
        mode="softmax": weight exp((score - best score) / temperature) for a valid candidate — exactly 1.0 for the best —, 0.0 for
        an invalid one (temperature > 0 and finite).
        Returns {"score": [M, B] float32, "weight": [M, B] float32, "top": [top, B] int32}: top[r, e] is the candidate at position r
        of env e's order (what draw_plans(index=) takes), -1 where the env has fewer valid candidates; 0 <= top <= 64, and with top=0
        there is no "top" entry.  An env without a valid candidate has weight 0 everywhere, which refit_plans() leaves unwritten.
        out: a dict with contiguous device tensors of those names, shapes and dtypes to write into; with it the method allocates
        nothing, without it exactly its results.  No two of the tensors may share memory (refused by the library).  The method reads
        no action and no state, so it works on discrete-action envs too."""
        torch = self.torch
        dev = self.device
        on_device = self._on_device
        on_device(seg_reward, (torch.float32,), None, "seg_reward")
        if seg_reward.dim() != 3 or int(seg_reward.shape[2]) != self.B:
            raise ValueError("seg_reward must be [M, H, B] with B = %d, got %r" % (self.B, tuple(seg_reward.shape)))
        M, H = int(seg_reward.shape[0]), int(seg_reward.shape[1])
        if not 1 <= H <= L.PLAN_MAX_H:
            raise ValueError("1 <= H (seg_reward.shape[1]) <= %d" % L.PLAN_MAX_H)
        self._drawn_m(M, "M (seg_reward.shape[0])")
        R = int(top)
        if not 0 <= R <= L.SCORE_MAX_TOP:
            raise ValueError("0 <= top <= %d" % L.SCORE_MAX_TOP)
        if n_steps is not None:
            on_device(n_steps, (torch.int16, getattr(torch, "uint16", torch.int16)), (M, self.B), "n_steps")
        if mode not in ("elite", "softmax"):
            raise ValueError('mode must be "elite" or "softmax"')
        if not np.isfinite(float(gamma)) or abs(float(gamma)) > float(np.finfo(np.float32).max):
            raise ValueError("gamma must be finite")
        if mode == "elite":
            if elites is None or not 1 <= int(elites) <= M:
                raise ValueError("mode=\"elite\" needs 1 <= elites <= M")
            sc = _lib.AtcPlanScore(L.SCORE_ELITE, int(elites), float(gamma), 0.0)
        else:
            t32 = np.float32(temperature) if temperature is not None else np.float32(np.nan)
            if not (t32 > 0 and np.isfinite(t32)):
                raise ValueError("mode=\"softmax\" needs a temperature > 0 and finite (in float32)")
            sc = _lib.AtcPlanScore(L.SCORE_SOFTMAX, 0, float(gamma), float(t32))
        want = {"score": ((torch.float32,), (M, self.B)), "weight": ((torch.float32,), (M, self.B))}
        if R:
            want["top"] = ((torch.int32,), (R, self.B))
        res = self._results(out, want, want.keys(), others=True)   # (other names in `out`: let through, unread)
        with torch.cuda.device(dev):
            _lib.check(self._lib.atc_plan_score(self.sector.handle, self.B, H, M, seg_reward.data_ptr(),
                                                None if n_steps is None else n_steps.data_ptr(), C.byref(sc), res["score"].data_ptr(),
                                                res["weight"].data_ptr(), res["top"].data_ptr() if R else None, R, self._stream()))
        self._keep_score = (seg_reward, n_steps)   # the inputs outlive the launch (like _keep_refit)
        return res

    def _check_twin(self, other, what):
        """branch() / select(): `other` must be an AtcVecEnv of the same N and device whose sector blob and atc_params_t are byte-equal"""
        if not isinstance(other, AtcVecEnv):
            raise ValueError("%s must be an AtcVecEnv" % what)
        if other is self:
            raise ValueError("%s must be another env than this one" % what)
        if other.N != self.N or other.device != self.device:
            raise ValueError("%s must have this env's num_aircraft and device" % what)
        if other.host_mapped or self.host_mapped:
            raise ValueError("branch / select need device-resident envs (host_mapped=False)")
        a, b = self.compiled.blob32, other.compiled.blob32
        if a.shape != b.shape or a.tobytes() != b.tobytes():
            raise ValueError("%s must be built on the same sector (byte-equal blob)" % what)
        if bytes(self.params) != bytes(other.params):
            raise ValueError("%s must have byte-equal parameters (atc_params_t)" % what)

    def branch(self, actions, K, into):
        """Branch (atc_branch, include/atc_step.h): flies each of M candidate decisions per env for up to K steps — what
        step_skip(actions[m], K) does from the state this env is in NOW — and KEEPS every outcome: candidate m of env e becomes env
        m * B + e of `into`, an AtcVecEnv with into.B == M * self.B, the same num_aircraft, device, sector and parameters (anything
        else: ValueError).  actions: [M, B, N, 3] (or [M, B, N*3]), 1 <= M <= 64, 1 <= K <= 255.  One launch; this env is left
        exactly as it is.  The results land in `into`'s own bound tensors (obs, reward, done, flags, ac_reward / min_sep where it
        has them, frame_steps), `into.traffic` is refreshed when it has one, and (obs, reward, done, info) of `into` is returned as
        step_skip returns it: view the tensors as [M, B, ...].  `into.raw_obs` and `into.term_obs` are NOT written (atc_lookahead_out_t has
        neither): they keep what they held.  An env-candidate with a WIDE heading is not evaluated: frame_steps
        == 0, zeros, and the child env is a copy of this env's.  For into.step(a, held=True) afterwards, the previous step of child
        m * B + e is this call's step with actions[m]; of a child that was not evaluated, the previous step of this env's env e.
        AtcSBVecEnv and AtcGym deliberately have no such method."""
        torch = self.torch
        K = self._held_k(K)
        M = int(actions.shape[0]) if hasattr(actions, "shape") else len(actions)
        if not 1 <= M <= L.LOOKAHEAD_MAX_M:
            raise ValueError("1 <= M (actions.shape[0]) <= %d" % L.LOOKAHEAD_MAX_M)
        self._check_twin(into, "into")
        if into.B != M * self.B:
            raise ValueError("into.num_envs must be M * num_envs = %d, got %d" % (M * self.B, into.B))
        a = self._as_actions(actions, lead=(M,))
        if into._info_skip is None:
            into._bind_frame_steps()
        out = _lib.AtcLookaheadOut(**{n: into._ptr(t) for n, t in (("reward", into.reward), ("done", into.done), ("n_steps", into.frame_steps),
                                                                   ("flags", into.flags), ("ac_reward", into.ac_reward),
                                                                   ("min_sep", into.min_sep), ("obs", into.obs))})
        with torch.cuda.device(self.device):
            _lib.check(self._lib.atc_branch(self.sector.handle, self.B, self.N, K, M, C.byref(self._state), self._ptr(a), C.byref(into._state),
                                            C.byref(out), C.byref(self.params), self._stream()))
            into._launch_traffic()
        into._prev_actions = None   # (check_held: the child's next step() has no previous step of its own to repeat)
        self._keep_branch = a   # the actions outlive the launch on a non-default stream (one tensor per call kind, like _keep_lookahead)
        return into.obs, into.reward, into.done, into._info_skip

    def select(self, src, index, mask=None):
        """State gather (atc_state_select, include/atc_step.h): env e of this batch takes the state of env index[e] of `src` — commit a
        branch()'s winner, keep a beam, restore a snapshot.  src: an AtcVecEnv of the same num_aircraft, device, sector and
        parameters (any num_envs); index: int32 / int64 tensor [B]; mask: optional [B], only envs with mask != 0 are written.  Envs
        masked out or with an index outside 0 .. src.B - 1 keep what they hold.  For the selected envs self.obs (and raw_obs where
        both envs have it) is gathered from src's as well — src's rows as they are: branch() does not write a child's raw_obs, so after
        branch(into=src) they are whatever src.raw_obs held before; self.traffic is refreshed when this env has one.  For
        step(a, held=True) afterwards, the previous step of a written env is the previous step of the src env it was gathered from; an
        env that was not written keeps its own.  Returns self.obs."""
        torch = self.torch
        self._check_twin(src, "src")
        index = self._as_tensor(index)
        if index.dtype not in (torch.int32, torch.int64) or index.numel() != self.B:
            raise ValueError("index must be an int32 / int64 tensor of %d elements" % self.B)
        idx = self._as_index(index, (self.B,), src.B)
        m = self._as_mask(mask)
        if m is not None and m.numel() != self.B:
            raise ValueError("mask must have %d elements" % self.B)
        with torch.cuda.device(self.device):
            _lib.check(self._lib.atc_state_select(self.sector.handle, self.N, self.B, C.byref(self._state), src.B, C.byref(src._state),
                                                  idx.data_ptr(), self._ptr(m), self._stream()))
            ok = (idx >= 0) & (idx < src.B)
            if m is not None:
                ok &= m.reshape(self.B) != 0
            rows = idx.clamp(0, src.B - 1).long()
            pairs = [(self.obs, src.obs)] + ([(self.raw_obs, src.raw_obs)] if self.raw_obs is not None and src.raw_obs is not None else [])
            for mine, theirs in pairs:
                mine.copy_(torch.where(ok[:, None], theirs.index_select(0, rows), mine))
            self._launch_traffic()
        self._prev_actions = None
        self._keep_select = (idx, m)   # (likewise: index and mask until the next select)
        return self.obs

    def make_launcher(self, actions, stream=None, held=False):
        """Pre-bound `atc_step` call for FIXED buffers (this env's state / outputs, the given device action tensor, the
        given torch stream or the current one): returns a no-argument callable that only launches — host cost of a few
        microseconds instead of the argument handling of step().  Meant for pipelined actors that keep several
        independent sub-batches in flight on separate streams (tools/multi_stream.py, bench.py --streams): a sub-batch's
        launch ramp and tail then overlap the others' bodies.  Results are in self.obs / reward / done / flags once the
        stream has reached the launch.  held=True passes the env's held-action parameter twin (ATC_M_ACTIONS_HELD set; the live
        object, so seed() / refresh_params() reach launchers that already exist): for the launches of a held action block after
        its first (see step()).  The promise itself — same actions as the previous launch, no set_last_action() in between —
        is the caller's and is not checked here (AtcVecEnv(check_held=True) checks it in step())."""
        torch = self.torch
        a = self._as_actions(actions)
        q = C.c_void_p((stream if stream is not None else torch.cuda.current_stream(self.device)).cuda_stream)
        params = self._params_held if held else self.params
        args = (self.sector.handle, self.B, self.N, C.byref(self._state), C.c_void_p(self._ptr(a)), C.byref(self._out),
                C.byref(params), q)
        fn, check = self._lib.atc_step, _lib.check

        def launch(_keep=(a, stream, params)):
            rc = fn(*args)
            if rc:
                check(rc)
        return launch

    def step_call(self, actions, stream=None, held=False):
        """The arguments of one atc_step of this env as an `atc_step_call_t` (+ the objects that must outlive it)."""
        a = self._as_actions(actions)
        q = (stream if stream is not None else self.torch.cuda.current_stream(self.device)).cuda_stream
        params = self._params_held if held else self.params   # the live objects, see make_launcher
        call = _lib.AtcStepCall(self.sector.handle, self.B, self.N, C.pointer(self._state), self._ptr(a),
                                C.pointer(self._out), C.pointer(params), q)
        return call, (a, stream, self, params)

    def step_async(self, actions):
        self._pending = actions

    def step_wait(self):
        return self.step(self._pending)

    def _info(self):
        info = {"flags": self.flags, "ep_return": self.ep_return, "ep_length": self.ep_length}
        if self.raw_obs is not None:
            info["original_state"] = self.raw_obs
        if self.ac_reward is not None:
            info["aircraft_reward"] = self.ac_reward
        if self.min_sep is not None:
            info["min_separation"] = self.min_sep
        if self.term_obs is not None:
            info["terminal_observation"] = self.term_obs
        if self.traffic is not None:
            info["traffic"] = self.traffic
        return info

    def rollout(self, actions, out=None, hold=1):
        """T consecutive steps in one launch (state stays in registers).  actions: [T / hold, B, N, 3]; each action block is
        applied for `hold` consecutive steps (frame skip, learning/atc-gym-demo.py:18-19), so T = hold * actions.shape[0].
        Returns a dict of [T, ...] device tensors (obs, reward, done, flags [+ optional outputs when `out` provides them]).
        A rollout does not produce the traffic observation (AtcVecEnv(traffic=K)): there is no [T, ...] traffic output, and
        self.traffic keeps what the last reset / observe / step left; call observe_traffic() afterwards for the final state."""
        torch = self.torch
        hold = int(hold)
        n_blocks = int(actions.shape[0])
        T = n_blocks * hold
        a = self._as_actions(actions, lead=(n_blocks,))
        B, N, dev = self.B, self.N, self.device
        if out is None:
            out = self._step_rows(T)
        o = self._make_out(out["obs"], out.get("raw_obs"), out["reward"], out.get("ac_reward"), out["done"],
                           out["flags"], out.get("min_sep"), out.get("term_obs"), None)
        with torch.cuda.device(dev):
            _lib.check(self._lib.atc_rollout_hold(self.sector.handle, B, N, T, hold, C.byref(self._state), self._ptr(a),
                                                  C.byref(o), C.byref(self.params), self._stream()))
        self._keep = a
        self._finish()
        return out

    def _step_rows(self, T):
        """fresh [T, ...] tensors for the four required outputs of T steps in one launch"""
        torch, B, N, dev = self.torch, self.B, self.N, self.device
        return {"obs": torch.empty((T, B, N * L.OBS_DIM), dtype=torch.float32, device=dev),
                "reward": torch.empty((T, B), dtype=torch.float32, device=dev),
                "done": torch.empty((T, B), dtype=torch.uint8, device=dev),
                "flags": torch.empty((T, B, N), dtype=torch.int16, device=dev)}

    def rollout_policy(self, weights, T, hold=1, seed=0, decision0=0, deterministic=False, obs0=None, out=None):
        """T consecutive steps in one launch with the decisions of a 10 -> 64 -> 64 -> 3 tanh MLP and a diagonal Gaussian taken inside
        it (include/atc_step.h: atc_rollout_policy) — the on-policy collection loop: observation -> policy -> sample -> clamp -> step.
        weights: the POLICY_WORDS-word float32 tensor of atc_hip.policy.pack_mlp / from_torch, on this env's device.  One decision per
        `hold` steps, each from the observation the step before it stored; decision 0 from `obs0` (default: the env's bound
        observation tensor, what the last reset / step left).  Successive calls pass decision0 += T // hold for fresh noise and the last
        row of the previous call's obs as obs0; deterministic=True flies the mean (logp = 0).
        Returns a dict of device tensors: obs / reward / done / flags [T, ...] as rollout() returns them, action [T // hold, B, N, 3] —
        the UNCLAMPED sample, what logp is about; its clamp to [-1, 1] is what was flown — and logp [T // hold, B, N].  Values are not
        computed: run the value network once over the stored obs.  Like rollout(), it produces no traffic observation: a policy that sees
        traffic is rolled out by rollout_policy_traffic(); rollout_policy_ends() also stores the terminal observations and the control mask."""
        return AtcVecEnv._rollout_policy(self, 0, weights, T, hold, seed, decision0, deterministic, obs0, out)

    def rollout_policy_traffic(self, weights, T, traffic, hold=1, seed=0, decision0=0, deterministic=False, obs0=None, out=None):
        """rollout_policy with a policy that also sees traffic (include/atc_step.h: atc_rollout_policy_traffic): at every decision each
        aircraft's `traffic` = K nearest intruders (1, 2 or 4) are found inside the launch, on the state as it is then, and words 0..6 of
        each record widen the input row to 10 + 7 K — exactly what observe_traffic() would return there, the convention of info["traffic"].
        weights: the L.policy_words(K)-word tensor of atc_hip.policy.pack_mlp / from_torch (traffic=K).  traffic=0 is rollout_policy itself.
        Returns rollout_policy's dict plus "traffic" [T // hold, B, N, K, 8], the records each decision saw (atc_hip.policy.input_rows builds
        the rows from them for the trainer's update); `out` may carry the buffers, "traffic" left out or None stores no records.
        Independent of the env's own traffic= setting: self.traffic is neither read nor written."""
        torch = self.torch
        K = int(traffic)
        if K == 0:
            return self.rollout_policy(weights, T, hold=hold, seed=seed, decision0=decision0, deterministic=deterministic, obs0=obs0, out=out)
        if K not in L.POLICY_TRAFFIC_K:
            raise ValueError("traffic must be 0 or one of %s records per aircraft" % (L.POLICY_TRAFFIC_K,))
        return AtcVecEnv._rollout_policy(self, K, weights, T, hold, seed, decision0, deterministic, obs0, out)   # (through the class: see gae)

    def rollout_policy_ends(self, weights, T, traffic=0, hold=1, seed=0, decision0=0, deterministic=False, obs0=None, out=None):
        """rollout_policy (traffic=0) or rollout_policy_traffic (traffic=K) through atc_rollout_policy_ends (include/atc_step.h), which adds
        what a trainer needs to treat episode ends and handed-over aircraft correctly and cannot rebuild from the [T, ...] tensors.  Per
        decision d = 0 .. T // hold - 1, whose ending step is the first step of its block with done set:
          term_obs [D, B, N, 10]: where block d has an ending step, the observation of the state that step ended in — what rollout()
            returns as term_obs there (the env has been reset inside that step, so obs holds the spawn observation).  Other rows are
            NOT written: a fresh tensor is zeros there, one given in `out` keeps its content;
          term_flags [D, B] int16: 0 where block d has no ending step, else L.TERM_ENDED | the OR of the env's flag words at that step
            (atc_hip.ppo.truncated() picks the time-limit ends);
          control [D, B, N] uint8: 1 where the aircraft was under control when decision d was taken.
        With out=, each of the three is stored only where `out` names it.  Every other output and the state afterwards are bit for bit
        those of the other two methods, which go through their own entry points as before."""
        K = int(traffic)
        if K and K not in L.POLICY_TRAFFIC_K:
            raise ValueError("traffic must be 0 or one of %s records per aircraft" % (L.POLICY_TRAFFIC_K,))
        return AtcVecEnv._rollout_policy(self, K, weights, T, hold, seed, decision0, deterministic, obs0, out, True)

    def rollout_policy_term(self, weights, T, traffic, hold=1, seed=0, decision0=0, deterministic=False, obs0=None, out=None):
        """rollout_policy_ends(traffic=K) for K = 1, 2 or 4 through atc_rollout_policy_term (include/atc_step.h), which also stores the traffic
        records of the state an episode ENDED in — the env is reset inside the ending step, so no later observe_traffic() can see it:
          term_traffic [D, B, N, K, 8]: where block d has an ending step, what observe_traffic() would return on the state term_obs[d]
            describes (after that step's kinematics and hand-overs, ahead of the spawn), bit for bit.  Like term_obs, other rows are NOT
            written: a fresh tensor is zeros there, one given in `out` keeps its content.
        atc_hip.policy.input_rows(term_obs, term_traffic) is then the row a critic over 10 + 7 K inputs bootstraps a time-limit end from
        (atc_hip.ppo.collect_bootstrap_traffic).  With out=, term_traffic is stored only where `out` names it, and nothing is allocated.
        Every other output and the state afterwards are rollout_policy_ends' bit for bit; that method goes through its own entry point."""
        K = int(traffic)
        if K not in L.POLICY_TRAFFIC_K:
            raise ValueError("traffic must be one of %s records per aircraft (a ten-word policy sees no records: rollout_policy_ends)" % (L.POLICY_TRAFFIC_K,))
        return AtcVecEnv._rollout_policy(self, K, weights, T, hold, seed, decision0, deterministic, obs0, out, True, True)

    def evaluate_policy(self, weights, T, traffic=0, hold=1, seed=0, decision0=0, deterministic=True, obs0=None, record=None, clear=True):
        """Flies the packed policy for T steps exactly as rollout_policy_ends() would — same decisions, same draws, same state afterwards —
        and stores none of its [T, ...] or [T // hold, ...] tensors (include/atc_step.h: atc_policy_eval).  What comes back is the per-env
        record, int32 [B, L.EVAL_WORDS]: episodes finished, wins, ends by cause, the finished episodes' summed length, return sum / sum of
        squares / min / max (float32 bit patterns: record[:, L.EVAL_RETURN_SUM].view(torch.float32)), the OR of every flag word seen, and
        the steps flown; atc_hip.evaluate.summary() folds it.  The record ACCUMULATES: clear=False adds this launch to what `record` holds,
        so chunks of a long evaluation chain — pass decision0 += T // hold and obs0 = the previous call's obs_last — and equal one launch
        bit for bit.  An episode that began before the call counts in full where it ends; one still running at the end is left in the env.
        The env must auto-reset.  obs0: default the env's bound observation tensor; a copy is taken.  Returns {"record", "obs_last"}."""
        torch = self.torch
        K, T, hold = int(traffic), int(T), int(hold)
        B, N, dev = self.B, self.N, self.device
        if K and K not in L.POLICY_TRAFFIC_K:
            raise ValueError("traffic must be 0 or one of %s records per aircraft" % (L.POLICY_TRAFFIC_K,))
        w, words = weights, L.policy_words(K) if K else L.POLICY_WORDS
        if not (torch.is_tensor(w) and w.dtype == torch.float32 and w.device == dev and w.is_contiguous() and w.numel() == words):
            raise ValueError("weights must be the contiguous float32 tensor of %d words (atc_hip.policy.pack_mlp%s) on %s" % (
                words, "(traffic=%d)" % K if K else "", dev))
        x0 = self.obs if obs0 is None else obs0
        if not (torch.is_tensor(x0) and x0.dtype == torch.float32 and x0.is_contiguous() and x0.numel() == B * N * L.OBS_DIM):
            raise ValueError("obs0 must be a contiguous float32 tensor of B*N*%d words" % L.OBS_DIM)
        x0 = x0.clone()
        if record is None:
            if not clear:
                raise ValueError("clear=False needs the record to add to")
            record = torch.empty((B, L.EVAL_WORDS), dtype=torch.int32, device=dev)
        elif not (torch.is_tensor(record) and record.dtype == torch.int32 and record.device == dev and record.is_contiguous() and record.numel() == B * L.EVAL_WORDS):
            raise ValueError("record must be a contiguous int32 tensor of [B, %d] on %s" % (L.EVAL_WORDS, dev))
        obs_last = torch.empty((B, N * L.OBS_DIM), dtype=torch.float32, device=dev)
        o = _lib.AtcPolicyEvalOut(self._ptr(record), self._ptr(obs_last), L.EVAL_CLEAR if clear else 0)
        pol = _lib.AtcPolicyTraffic(self._ptr(w), L.POLICY_HIDDEN, L.POLICY_DETERMINISTIC if deterministic else 0, int(seed) & (2 ** 64 - 1),
                                    int(decision0) & 0xffffffff, 0, K)
        with torch.cuda.device(dev):
            rc = self._lib.atc_policy_eval(self.sector.handle, B, N, T, hold, C.byref(self._state), self._ptr(x0), C.byref(pol), C.byref(o),
                                           C.byref(self.params), self._stream())
            if rc:
                _lib.check(rc)
        self._keep = (w, x0)
        if self.host_mapped:
            self._finish()
        return {"record": record, "obs_last": obs_last}

    def _rollout_policy(self, K, weights, T, hold, seed, decision0, deterministic, obs0, out, ends=False, term=False):
        """rollout_policy (K = 0) and rollout_policy_traffic (K = 1, 2, 4): the checks of weights and obs0, the result tensors, the two
        structs, the launch.  ends: through atc_rollout_policy_ends, with its three further outputs; term (with ends, K > 0): through
        atc_rollout_policy_term, with term_traffic behind them"""
        torch = self.torch
        T, hold = int(T), int(hold)
        B, N, dev = self.B, self.N, self.device
        w, words = weights, L.policy_words(K) if K else L.POLICY_WORDS
        if not (torch.is_tensor(w) and w.dtype == torch.float32 and w.device == dev and w.is_contiguous() and w.numel() == words):
            raise ValueError("weights must be the contiguous float32 tensor of %d words (atc_hip.policy.pack_mlp%s) on %s" % (
                words, "(traffic=%d)" % K if K else "", dev))
        x0 = self.obs if obs0 is None else obs0
        if not (torch.is_tensor(x0) and x0.dtype == torch.float32 and x0.is_contiguous() and x0.numel() == B * N * L.OBS_DIM):
            raise ValueError("obs0 must be a contiguous float32 tensor of B*N*%d words" % L.OBS_DIM)
        if out is None or K or ends:
            n_dec = T // hold if hold >= 1 else 0     # (a T or hold the library refuses is refused by it, below)
        if out is None:
            out = self._step_rows(T)
            out["action"] = torch.empty((n_dec, B, N, L.ACT_DIM), dtype=torch.float32, device=dev)
            out["logp"] = torch.empty((n_dec, B, N), dtype=torch.float32, device=dev)
            if K:
                out["traffic"] = torch.empty((n_dec, B, N, K, L.TRAFFIC_DIM), dtype=torch.float32, device=dev)
            if ends:   # (term_obs: zeros, since the rows of a block without an ending step are not written)
                out["term_obs"] = torch.zeros((n_dec, B, N, L.OBS_DIM), dtype=torch.float32, device=dev)
                out["term_flags"] = torch.empty((n_dec, B), dtype=torch.int16, device=dev)
                out["control"] = torch.empty((n_dec, B, N), dtype=torch.uint8, device=dev)
            if term:   # (zeros, like term_obs)
                out["term_traffic"] = torch.zeros((n_dec, B, N, K, L.TRAFFIC_DIM), dtype=torch.float32, device=dev)
        if ends:
            for name, dtype, shape in (("term_obs", torch.float32, (n_dec, B, N, L.OBS_DIM)), ("term_flags", torch.int16, (n_dec, B)),
                                       ("control", torch.uint8, (n_dec, B, N))) + ((("term_traffic", torch.float32, (n_dec, B, N, K, L.TRAFFIC_DIM)),) if term else ()):
                t = out.get(name)
                if t is not None and not (torch.is_tensor(t) and t.dtype == dtype and t.device == dev and t.is_contiguous() and t.numel() == int(np.prod(shape))):
                    raise ValueError("out[%r] must be a contiguous %s tensor of %r on %s" % (name, dtype, shape, dev))
        if K:
            tr = out.get("traffic")
            if tr is not None and not (torch.is_tensor(tr) and tr.dtype == torch.float32 and tr.is_contiguous() and tr.numel() == n_dec * B * N * K * L.TRAFFIC_DIM):
                raise ValueError("out['traffic'] must be a contiguous float32 tensor of [T // hold, B, N, %d, %d]" % (K, L.TRAFFIC_DIM))
            call, pol_type, out_type, fields = self._lib.atc_rollout_policy_traffic, _lib.AtcPolicyTraffic, _lib.AtcPolicyTrafficOut, _lib.POLICY_TRAFFIC_OUT_FIELDS
        else:
            call, pol_type, out_type, fields = self._lib.atc_rollout_policy, _lib.AtcPolicy, _lib.AtcPolicyOut, _lib.POLICY_OUT_FIELDS
        if ends:
            call, pol_type, out_type, fields = self._lib.atc_rollout_policy_ends, _lib.AtcPolicyTraffic, _lib.AtcPolicyEndsOut, _lib.POLICY_ENDS_OUT_FIELDS
        if term:
            call, out_type, fields = self._lib.atc_rollout_policy_term, _lib.AtcPolicyTermOut, _lib.POLICY_TERM_OUT_FIELDS
        o =out_type(*[self._ptr(out.get(k)) if (K or k != "traffic") else None for k in fields])
        pol = pol_type(self._ptr(w), L.POLICY_HIDDEN, L.POLICY_DETERMINISTIC if deterministic else 0, int(seed) & (2 ** 64 - 1),
                       int(decision0) & 0xffffffff, 0)     # (traffic_k, where the struct has it, is zero so far)
        if K:
            pol.traffic_k = K
        with torch.cuda.device(dev):
            rc = call(self.sector.handle, B, N, T, hold, C.byref(self._state), self._ptr(x0), C.byref(pol), C.byref(o), C.byref(self.params), self._stream())
            if rc:
                _lib.check(rc)
        self._keep = (w, x0)
        if self.host_mapped:
            self._finish()
        return out

    def gae(self, reward, done, values, hold=1, gamma=0.99, lam=0.95, *, per_decision=False, adv_next=None, out=None):
        """Advantages and returns of a collection in one launch on this env's current stream (atc_gae, include/atc_step.h): what lies
        between rollout_policy() plus one value forward and the update.  reward: [T, B] float32 and done: [T, B] uint8 as rollout_policy()
        returns them, values: [D + 1, B, NV] float32 ([D + 1, B] means NV = 1) with T = D * hold — row d the value of the state decision d
        was taken in, row D the value of the state after the last step; 1 <= NV <= 64.  All contiguous tensors on this env's device
        (nothing is converted: ValueError otherwise).  reward [T, B, NV] gives every value column its own reward (a per-aircraft reward).
        A decision's `hold` steps become ONE transition: R = r_0 + r_1 gamma + r_2 gamma^2 + ... (fp32, left to right, the discount a
        running product) up to and including the block's first done — the steps behind it belong to the next episode and are not read
        into anything — and the decisions are discounted with G = gamma^hold.  per_decision=True: R is the plain sum and G = gamma, what
        a frame-skipping env in front of a trainer computes.  Then, d descending, with A_next = adv_next ([B, NV], default zeros):
        a block that ended its episode has A = R - V[d], any other A = (R + G V[d+1]) - V[d] + (G lam) A_next; ret = A + V[d].
        Returns {"adv", "ret": [D, B, NV] float32, "block_reward": [D, B] float32 ([D, B, NV] with a per-column reward), "block_done",
        "block_steps": [D, B] uint8} (the [.., NV] axis is left out where values has none).  out: a dict with contiguous device tensors of
        those names, shapes and dtypes to write into — "adv" and "ret" required, the three block outputs stored only where it names
        them; with it the method allocates nothing.  No two of the tensors may share memory (refused by the library).  Two calls split
        at D / 2, the later half first and its adv[0] as the earlier half's adv_next, equal one call bit for bit.
        Every done is a true terminal state here: gae_boot() bootstraps a time-limit done from the terminal observation that
        rollout_policy_ends() stores, next to the mask of the aircraft that were not under control.  Not covered, the trainer's: advantage
        normalisation (with that mask, three reductions over [D, B, N]) and the traffic records of a terminal state.  The method reads no
        action and no state."""
        return AtcVecEnv._gae(self, reward, done, values, hold, gamma, lam, per_decision, adv_next, out, None, None)

    def gae_boot(self, reward, done, values, boot, trunc, hold=1, gamma=0.99, lam=0.95, *, per_decision=False, adv_next=None, out=None):
        """gae() with bootstrapped truncations (atc_gae_boot, include/atc_step.h).  boot: [D, B, NV] float32 ([D, B] where values is) and
        trunc: [D, B] uint8, contiguous on this env's device, both or neither (None, None is gae() through atc_gae_boot; one without the
        other: ValueError).  A block that ended its episode with trunc[d, e] != 0 — a time-limit end: atc_hip.ppo.truncated() of
        rollout_policy_ends()'s term_flags — bootstraps from boot[d], the critic's value of term_obs[d]:
        A = (R + Gn boot[d]) - V[d] with Gn = gamma^(steps the block counted) (gamma with per_decision); A_next does not enter, the episode
        still ends there.  A boot word anywhere else is not read into anything (a NaN may stand there).  Everything else is gae()'s."""
        if (boot is None) != (trunc is None):
            raise ValueError("boot and trunc go together: both or neither")
        return AtcVecEnv._gae(self, reward, done, values, hold, gamma, lam, per_decision, adv_next, out, boot, trunc, True)

    def _gae(self, reward, done, values, hold, gamma, lam, per_decision, adv_next, out, boot, trunc, through_boot=False):
        """gae() and gae_boot(): the checks, the result tensors, the two structs, the launch"""
        torch = self.torch
        dev, f32 = self.device, (self.torch.float32,)
        # (the helpers through the class: these refusals are also tested on a stand-in env that has none of the class's methods)
        need = AtcVecEnv._on_device.__get__(self)
        hold = int(hold)
        if not 1 <= hold <= L.SKIP_MAX:
            raise ValueError("1 <= hold <= %d" % L.SKIP_MAX)
        if not (torch.is_tensor(values) and values.dim() in (2, 3) and int(values.shape[0]) >= 2 and int(values.shape[1]) == self.B):
            raise ValueError("values must be [D + 1, B, NV] or [D + 1, B] with D >= 1 and B = %d" % self.B)
        D = int(values.shape[0]) - 1
        NV = int(values.shape[2]) if values.dim() == 3 else 1
        if not 1 <= NV <= L.GAE_MAX_NV:
            raise ValueError("1 <= NV (values.shape[-1]) <= %d" % L.GAE_MAX_NV)
        cols = tuple(values.shape[1:])
        need(values, f32, (D + 1,) + cols, "values")
        T = D * hold
        if not torch.is_tensor(reward) or reward.dim() not in (2, 3):
            raise ValueError("reward must be [T, B] or [T, B, NV]")
        per_column = reward.dim() == 3
        need(reward, f32, (T, self.B, NV) if per_column else (T, self.B), "reward")
        need(done, (torch.uint8,), (T, self.B), "done")
        for name, v in (("gamma", gamma), ("lam", lam)):
            with np.errstate(over="ignore"):
                if not np.isfinite(np.float32(v)):
                    raise ValueError("%s must be finite (in float32)" % name)
        if adv_next is not None:
            need(adv_next, f32, cols, "adv_next")
        if boot is not None:
            need(boot, f32, (D,) + cols, "boot")
            need(trunc, (torch.uint8,), (D, self.B), "trunc")
        want = {"adv": (f32, (D,) + cols), "ret": (f32, (D,) + cols), "block_reward": (f32, (D,) + (cols if per_column else (self.B,))),
                "block_done": ((torch.uint8,), (D, self.B)), "block_steps": ((torch.uint8,), (D, self.B))}
        res = AtcVecEnv._results(self, out, want, {"adv", "ret"}, "out must be a dict with adv and ret, and any of block_reward, block_done, block_steps")
        g = _lib.AtcGae(float(gamma), float(lam), (L.GAE_PER_DECISION if per_decision else 0) | (L.GAE_REWARD_PER_COLUMN if per_column else 0), 0)
        o = _lib.AtcGaeOut(*[res[n].data_ptr() if n in res else None for n in _lib.GAE_OUT_FIELDS])
        fn = self._lib.atc_gae_boot if through_boot else self._lib.atc_gae
        with torch.cuda.device(dev):
            extra = (None if boot is None else boot.data_ptr(), None if trunc is None else trunc.data_ptr()) if through_boot else ()
            rc = fn(self.sector.handle, self.B, NV, D, hold, reward.data_ptr(), done.data_ptr(), values.data_ptr(),
                    None if adv_next is None else adv_next.data_ptr(), *extra, C.byref(g), C.byref(o), self._stream())
            if rc:
                _lib.check(rc)
        self._keep_gae = (reward, done, values, adv_next, boot, trunc)   # the inputs outlive the launch (like _keep_score)
        return res

    def ppo_policy_grad(self, weights, obs_rows, action, logp_old, adv, *, traffic=None, mask=None, index=None, clip=0.2, adv_shift=0.0,
                        adv_scale=1.0, workgroups=0, out=None):
        """The PPO policy loss and its gradient with respect to the packed weights in one call on this env's current stream
        (atc_ppo_policy_grad, include/atc_step.h): the policy half of an update is `w.grad = env.ppo_policy_grad(...)["grad"]` and the
        trainer's own optimiser on the packed tensor; no activation is written to memory.  Over R_src stored decisions:
        weights: the L.policy_words(K)-word tensor of atc_hip.policy.pack_mlp; obs_rows [..., 10]: what each decision saw; traffic
        [..., K, 8] (K = 1, 2, 4) the records it saw — words 0..6 widen the row as atc_hip.policy.input_rows does — or None for the
        ten-word policy; action [..., 3]: the UNCLAMPED sample; logp_old, adv: [...] float32; mask: uint8 of R_src elements or None
        (rollout_policy_ends' control); index: int32 [R] or None — the minibatch: row i evaluates source row index[i], an index outside
        0 .. R_src - 1 is skipped.  All contiguous tensors on this env's device; nothing is converted (ValueError otherwise).
        Per row that takes part: ratio = exp(logp - logp_old), A = (adv - adv_shift) * adv_scale (normalisation stays the trainer's: it
        passes the two scalars), L = -min(ratio A, clamp(ratio, 1 - clip, 1 + clip) A), and the gradient torch.autograd gives for it.
        Returns {"grad": [policy_words(K)] — the mean over the n rows that take part, zeros if there is none —, "stats": [8] (the
        L.PPO_STAT_* words: n, mean L, mean (logp_old - logp), the fraction of rows whose gradient was cut, mean ratio,
        max |logp - logp_old|, two zeros), "logp": [R], written where a row takes part (NaN elsewhere in a fresh tensor; a tensor given in
        `out` keeps what it holds there)}.  out: a dict with any of "grad", "stats", "logp" and "scratch" ([G, policy_words(K) + 8] float32
        with G = L.ppo_grad_workgroups(R, workgroups)); with all four the method allocates nothing.  workgroups: 0, or the number G of
        workgroups, 1 .. L.PPO_GRAD_MAX_WG — the same inputs and the same G give the same bits on every run.  No output may share memory
        with another tensor of the call (refused by the library).
        Not in this call: the value loss (ppo_value_grad, on a critic packed by atc_hip.value); the trainer's: the entropy bonus
        (sum(log_std) + a constant) and the optimiser, stepped on the two packed tensors."""
        torch = self.torch
        dev, f32 = self.device, (self.torch.float32,)
        need = AtcVecEnv._on_device.__get__(self)
        K = 0
        if traffic is not None:
            if not (torch.is_tensor(traffic) and traffic.dim() >= 3 and int(traffic.shape[-1]) == L.TRAFFIC_DIM and int(traffic.shape[-2]) in L.POLICY_TRAFFIC_K):
                raise ValueError("traffic must be [..., K, %d] with K one of %s records per aircraft, or None" % (L.TRAFFIC_DIM, L.POLICY_TRAFFIC_K))
            K = int(traffic.shape[-2])
        words = L.policy_words(K)
        need(weights, f32, (words,), text="weights must be the contiguous float32 tensor of %r words (atc_hip.policy.pack_mlp) on %s", elements=True)
        if not (torch.is_tensor(obs_rows) and obs_rows.dim() >= 1 and int(obs_rows.shape[-1]) == L.OBS_DIM and obs_rows.numel() >= L.OBS_DIM):
            raise ValueError("obs_rows must be [..., %d] with at least one row" % L.OBS_DIM)
        R_src = obs_rows.numel() // L.OBS_DIM
        if R_src > 2 ** 31 - 1:
            raise ValueError("obs_rows holds more rows than one call covers (2^31 - 1)")
        need(obs_rows, f32, (R_src, L.OBS_DIM), "obs_rows", elements=True)
        if traffic is not None:
            need(traffic, f32, (R_src, K, L.TRAFFIC_DIM), "traffic", elements=True)
        if not (torch.is_tensor(action) and action.dim() >= 1 and int(action.shape[-1]) == L.ACT_DIM):
            raise ValueError("action must be [..., %d]" % L.ACT_DIM)
        need(action, f32, (R_src, L.ACT_DIM), "action", elements=True)
        need(logp_old, f32, (R_src,), "logp_old", elements=True)
        need(adv, f32, (R_src,), "adv", elements=True)
        if mask is not None:
            need(mask, (torch.uint8,), (R_src,), "mask", elements=True)
        R = R_src
        if index is not None:
            if not (torch.is_tensor(index) and index.dim() == 1 and 1 <= index.numel() <= 2 ** 31 - 1):
                raise ValueError("index must be an int32 tensor [R] with R >= 1")
            R = int(index.numel())
            need(index, (torch.int32,), (R,), "index")
        with np.errstate(over="ignore"):
            if not (np.isfinite(np.float32(clip)) and np.float32(clip) > 0):
                raise ValueError("clip must be finite (in float32) and > 0")
        workgroups = int(workgroups)
        if not 0 <= workgroups <= L.PPO_GRAD_MAX_WG:
            raise ValueError("0 <= workgroups <= %d" % L.PPO_GRAD_MAX_WG)
        G = L.ppo_grad_workgroups(R, workgroups)
        want = {"grad": (f32, (words,)), "stats": (f32, (L.PPO_GRAD_STATS,)), "logp": (f32, (R,)), "scratch": (f32, (G, words + L.PPO_GRAD_STATS))}
        if out is None:
            res = {"grad": torch.empty(words, dtype=torch.float32, device=dev), "stats": torch.empty(L.PPO_GRAD_STATS, dtype=torch.float32, device=dev),
                   "logp": torch.full((R,), float("nan"), dtype=torch.float32, device=dev)}
        else:
            res = AtcVecEnv._results(self, out, want, set(), "out must be a dict with any of grad, stats, logp, scratch")
            for n in ("grad", "stats"):
                if n not in res:
                    res[n] = torch.empty(want[n][1], dtype=torch.float32, device=dev)
            if "logp" not in res:
                res["logp"] = torch.full((R,), float("nan"), dtype=torch.float32, device=dev)
        scratch = res.pop("scratch", None)
        if scratch is None:
            scratch = torch.empty((G, words + L.PPO_GRAD_STATS), dtype=torch.float32, device=dev)
        g = _lib.AtcPpoGrad(K, float(clip), float(adv_shift), float(adv_scale), workgroups, 0)
        o = _lib.AtcPpoGradOut(res["grad"].data_ptr(), res["stats"].data_ptr(), res["logp"].data_ptr(), scratch.data_ptr())
        fn = self._lib.atc_ppo_policy_grad
        with torch.cuda.device(dev):
            rc = fn(self.sector.handle, R_src, R, weights.data_ptr(), obs_rows.data_ptr(),
                                               None if traffic is None else traffic.data_ptr(), action.data_ptr(), logp_old.data_ptr(), adv.data_ptr(),
                                               None if mask is None else mask.data_ptr(), None if index is None else index.data_ptr(),
                                               C.byref(g), C.byref(o), self._stream())
            if rc:
                _lib.check(rc)
        self._keep_ppo_grad = (weights, obs_rows, traffic, action, logp_old, adv, mask, index, scratch)   # they outlive the two launches
        return res

    def value_forward(self, weights, rows, *, out=None):
        """V of every row in one launch on this env's current stream (atc_value_forward, include/atc_step.h): the critic of atc_hip.value —
        (10 + 7 K) -> 64 -> 64 -> 1, tanh — evaluated one lane per row, no activation written to memory.
        weights: the L.value_words(K)-word tensor of atc_hip.value.pack_mlp; rows [..., IN] float32, contiguous, on this env's device, with
        IN = 10 + 7 K for K = 0, 1, 2 or 4: the rows as atc_hip.ppo.value_rows() makes them (atc_hip.policy.input_rows widens them).  Nothing
        is converted (ValueError otherwise).  Returns a float32 tensor of shape rows.shape[:-1]; out: that tensor, and nothing is allocated."""
        torch = self.torch
        f32 = (torch.float32,)
        need = AtcVecEnv._on_device.__get__(self)
        ins = {L.policy_in(k): k for k in (0,) + L.POLICY_TRAFFIC_K}
        if not (torch.is_tensor(rows) and rows.dim() >= 1 and int(rows.shape[-1]) in ins and rows.numel() >= int(rows.shape[-1])):
            raise ValueError("rows must be [..., IN] with IN one of %s (10 + 7 K) and at least one row" % (sorted(ins),))
        IN = int(rows.shape[-1])
        K = ins[IN]
        R = rows.numel() // IN
        if R > 2 ** 31 - 1:
            raise ValueError("rows holds more rows than one call covers (2^31 - 1)")
        need(rows, f32, (R, IN), "rows", elements=True)
        need(weights, f32, (L.value_words(K),), text="weights must be the contiguous float32 tensor of %r words (atc_hip.value.pack_mlp) on %s", elements=True)
        shape = tuple(rows.shape[:-1])
        if out is None:
            out = torch.empty(shape, dtype=torch.float32, device=self.device)
        else:
            need(out, f32, shape, "out")
        fn = self._lib.atc_value_forward
        with torch.cuda.device(self.device):
            rc = fn(self.sector.handle, R, K, weights.data_ptr(), rows.data_ptr(), out.data_ptr(), self._stream())
            if rc:
                _lib.check(rc)
        self._keep_value = (weights, rows, out)      # they outlive the launch
        return out

    POLICY_FORWARD_OUTPUTS = ("mean", "action", "flown", "logp")

    def policy_forward(self, weights, obs_rows, *, traffic=None, samples=1, rows_per_decision=None, seed=0, decision0=0, deterministic=False,
                       outputs=("flown", "logp"), out=None):
        """The decisions of the packed policy on given rows, outside a rollout, in one launch on this env's current stream
        (atc_policy_forward, include/atc_step.h): the MLP once per row in the rollout's arithmetic, then `samples` draws per row.
        weights: the L.policy_words(K)-word tensor of atc_hip.policy.pack_mlp — K is found from its size; obs_rows [..., 10]: the own
        observation rows; traffic [..., K, 8] for K > 0 (words 0..6 of each record widen the row; env.traffic and the rollout's stored
        records are taken as they are), None for K = 0.  Contiguous float32 tensors on this env's device; nothing is converted.
        Sample s of row r is drawn with the rollout's key of decision = decision0 + s * ceil(R / P) + r // P and aircraft r % P, with
        P = rows_per_decision (default: all R rows are one decision): with P = B * N the rows [D, B, N] a rollout's decisions saw get the
        rollout's draws.  deterministic=True: action = mean, logp = 0, samples must be 1.
        Returns a dict of the names in `outputs`, any of "mean" [..., 3], "action" [S, ..., 3] (the UNCLAMPED sample), "flown" [S, ..., 3]
        (its clamp to [-1, 1]: what step / step_skip / lookahead / branch take) and "logp" [S, ...].  out: a dict of those tensors — its
        keys are the outputs, and nothing is allocated."""
        torch = self.torch
        f32 = (torch.float32,)
        need = AtcVecEnv._on_device.__get__(self)
        if not (torch.is_tensor(weights) and weights.dim() >= 1):
            raise ValueError("weights must be the packed float32 tensor of atc_hip.policy.pack_mlp")
        K = policy.traffic_of(weights.numel())
        need(weights, f32, (L.policy_words(K),), text="weights must be the contiguous float32 tensor of %r words (atc_hip.policy.pack_mlp) on %s", elements=True)
        if not (torch.is_tensor(obs_rows) and obs_rows.dim() >= 1 and int(obs_rows.shape[-1]) == L.OBS_DIM and obs_rows.numel() >= L.OBS_DIM):
            raise ValueError("obs_rows must be [..., %d] with at least one row" % L.OBS_DIM)
        lead = tuple(obs_rows.shape[:-1])
        R = obs_rows.numel() // L.OBS_DIM
        if R > 2 ** 31 - 1:
            raise ValueError("obs_rows holds more rows than one call covers (2^31 - 1)")
        need(obs_rows, f32, (R, L.OBS_DIM), "obs_rows", elements=True)
        if K:
            if not (torch.is_tensor(traffic) and traffic.dim() >= 2 and tuple(traffic.shape[-2:]) == (K, L.TRAFFIC_DIM)):
                raise ValueError("traffic must be [..., %d, %d]: these weights are a policy that sees %d records per aircraft" % (K, L.TRAFFIC_DIM, K))
            need(traffic, f32, (R, K, L.TRAFFIC_DIM), "traffic", elements=True)
        elif traffic is not None:
            raise ValueError("traffic must be None: these weights are the ten-word policy")
        S = int(samples)
        if not 1 <= S <= L.POLICY_FWD_MAX_SAMPLES:
            raise ValueError("1 <= samples <= %d" % L.POLICY_FWD_MAX_SAMPLES)
        if deterministic and S != 1:
            raise ValueError("deterministic=True draws nothing: samples must be 1")
        P = R if rows_per_decision is None else int(rows_per_decision)
        if not 1 <= P <= R:
            raise ValueError("1 <= rows_per_decision <= the number of rows (%d)" % R)
        want = {"mean": (f32, lead + (L.ACT_DIM,)), "action": (f32, (S,) + lead + (L.ACT_DIM,)), "flown": (f32, (S,) + lead + (L.ACT_DIM,)),
                "logp": (f32, (S,) + lead)}
        if out is None:
            names = (outputs,) if isinstance(outputs, str) else tuple(outputs)
            if not names or any(n not in want for n in names):
                raise ValueError("outputs must name at least one of %s" % ", ".join(want))
            res = {n: torch.empty(want[n][1], dtype=torch.float32, device=self.device) for n in names}
        else:
            if not isinstance(out, dict) or not out:
                raise ValueError("out must be a dict with any of %s" % ", ".join(want))
            res = AtcVecEnv._results(self, out, want, set(), "out must be a dict with any of %s" % ", ".join(want))
        f = _lib.AtcPolicyFwd(K, S, P, L.POLICY_DETERMINISTIC if deterministic else 0, int(seed) & (2 ** 64 - 1), int(decision0) & 0xffffffff, 0)
        o = _lib.AtcPolicyFwdOut(*[res[n].data_ptr() if n in res else None for n in _lib.POLICY_FWD_OUT_FIELDS])
        fn = self._lib.atc_policy_forward
        with torch.cuda.device(self.device):
            rc = fn(self.sector.handle, R, weights.data_ptr(), obs_rows.data_ptr(), traffic.data_ptr() if K else None, C.byref(f), C.byref(o),
                    self._stream())
            if rc:
                _lib.check(rc)
        self._keep_policy_forward = (weights, obs_rows, traffic, res)      # they outlive the launch
        return res

    def act(self, weights, *, samples=None, seed=0, decision=0, deterministic=False, out=None):
        """The packed policy's decision for the state the env is in NOW (policy_forward on env.obs and, for a policy that sees traffic,
        env.traffic — the env must have been made with that traffic=K): what rollout_policy(weights, hold, hold=hold, seed=seed,
        decision0=decision) would fly from here.  Returns flown, [B, N, 3] — or [M, B, N, 3] with samples=M, M candidates per aircraft —:
        exactly what step / step_skip / lookahead / branch take.  out: that tensor, and nothing is allocated."""
        torch = self.torch
        AtcVecEnv._refuse_discrete(self)
        if not torch.is_tensor(weights):
            raise ValueError("weights must be the packed float32 tensor of atc_hip.policy.pack_mlp")
        K = policy.traffic_of(weights.numel())
        if K != self.traffic_k:
            raise ValueError("these weights are a policy that sees %d traffic records per aircraft, this env observes %d (AtcVecEnv(traffic=%d))" % (
                K, self.traffic_k, K))
        B, N = self.B, self.N
        S = 1 if samples is None else int(samples)
        shape = (B, N, L.ACT_DIM) if samples is None else (S, B, N, L.ACT_DIM)
        if out is not None:
            AtcVecEnv._on_device(self, out, (torch.float32,), shape, "out")
        rows = self.obs.view(B, N, L.OBS_DIM)
        if not rows.is_cuda:      # (a host-mapped env's observation lives in pinned host memory)
            rows = rows.to(self.device)
        tr = self.traffic
        if K and not tr.is_cuda:
            tr = tr.to(self.device)
        res = AtcVecEnv.policy_forward(self, weights, rows, traffic=tr if K else None, samples=S, rows_per_decision=B * N, seed=seed,
                                       decision0=decision, deterministic=deterministic,
                                       out={"flown": (out if samples is not None else out.view((1,) + shape))} if out is not None else None,
                                       outputs=("flown",))
        return out if out is not None else (res["flown"] if samples is not None else res["flown"][0])

    def ppo_value_grad(self, weights, obs_rows, v_old, ret, *, traffic=None, mask=None, index=None, clip=0.2, workgroups=0, out=None):
        """The clipped PPO value loss and its gradient with respect to the packed critic in one call on this env's current stream
        (atc_ppo_value_grad, include/atc_step.h): the value half of an update is `vw.grad = env.ppo_value_grad(...)["grad"]` and the
        trainer's own optimiser on the packed tensor; no activation is written to memory.  Over R_src stored decisions:
        weights: the L.value_words(K)-word tensor of atc_hip.value.pack_mlp; obs_rows [..., 10], traffic [..., K, 8] or None, mask, index:
        as in ppo_policy_grad (read in place, a minibatch is gathered by `index` without a copy); v_old, ret: [...] float32 of R_src
        elements — the values the collection stored and its returns.  All contiguous tensors on this env's device.
        Per row that takes part, with v = V(row): e = v - ret, d = v - v_old, vc = v_old + clamp(d, -clip, clip); L = 0.5 e^2 and
        dL/dv = e where |d| <= clip or e^2 >= (vc - ret)^2, else the row is cut: L = 0.5 (vc - ret)^2, dL/dv = 0 — PPO2's
        0.5 max((v - ret)^2, (vc - ret)^2).  clip=float("inf") is the plain squared error.
        Returns {"grad": [value_words(K)] — the mean over the n rows that take part, zeros if there is none —, "stats": [8] (the
        L.PPO_VSTAT_* words: n, mean L, the fraction cut, mean v, mean ret, mean ret^2, mean (ret - v)^2, max |v - v_old|; words 4 .. 6 give
        the explained variance), "value": [R], written where a row takes part (NaN elsewhere in a fresh tensor; a tensor given in `out`
        keeps what it holds there) — bit for bit value_forward's output where the tiles of 64 rows hold the same rows}.  out: a dict with
        any of "grad", "stats", "value" and "scratch" ([G, value_words(K) + 8] float32 with G = L.ppo_grad_workgroups(R, workgroups)); with
        all four the method allocates nothing.  workgroups: as in ppo_policy_grad.  No output may share memory with another tensor of the
        call (refused by the library)."""
        torch = self.torch
        dev, f32 = self.device, (self.torch.float32,)
        need = AtcVecEnv._on_device.__get__(self)
        K = 0
        if traffic is not None:
            if not (torch.is_tensor(traffic) and traffic.dim() >= 3 and int(traffic.shape[-1]) == L.TRAFFIC_DIM and int(traffic.shape[-2]) in L.POLICY_TRAFFIC_K):
                raise ValueError("traffic must be [..., K, %d] with K one of %s records per aircraft, or None" % (L.TRAFFIC_DIM, L.POLICY_TRAFFIC_K))
            K = int(traffic.shape[-2])
        words = L.value_words(K)
        need(weights, f32, (words,), text="weights must be the contiguous float32 tensor of %r words (atc_hip.value.pack_mlp) on %s", elements=True)
        if not (torch.is_tensor(obs_rows) and obs_rows.dim() >= 1 and int(obs_rows.shape[-1]) == L.OBS_DIM and obs_rows.numel() >= L.OBS_DIM):
            raise ValueError("obs_rows must be [..., %d] with at least one row" % L.OBS_DIM)
        R_src = obs_rows.numel() // L.OBS_DIM
        if R_src > 2 ** 31 - 1:
            raise ValueError("obs_rows holds more rows than one call covers (2^31 - 1)")
        need(obs_rows, f32, (R_src, L.OBS_DIM), "obs_rows", elements=True)
        if traffic is not None:
            need(traffic, f32, (R_src, K, L.TRAFFIC_DIM), "traffic", elements=True)
        need(v_old, f32, (R_src,), "v_old", elements=True)
        need(ret, f32, (R_src,), "ret", elements=True)
        if mask is not None:
            need(mask, (torch.uint8,), (R_src,), "mask", elements=True)
        R = R_src
        if index is not None:
            if not (torch.is_tensor(index) and index.dim() == 1 and 1 <= index.numel() <= 2 ** 31 - 1):
                raise ValueError("index must be an int32 tensor [R] with R >= 1")
            R = int(index.numel())
            need(index, (torch.int32,), (R,), "index")
        with np.errstate(over="ignore"):
            if not np.float32(clip) > 0:
                raise ValueError("clip must be > 0 in float32 (float('inf'): no clipping) and not a NaN")
        workgroups = int(workgroups)
        if not 0 <= workgroups <= L.PPO_GRAD_MAX_WG:
            raise ValueError("0 <= workgroups <= %d" % L.PPO_GRAD_MAX_WG)
        G = L.ppo_grad_workgroups(R, workgroups)
        want = {"grad": (f32, (words,)), "stats": (f32, (L.PPO_VALUE_STATS,)), "value": (f32, (R,)), "scratch": (f32, (G, words + L.PPO_VALUE_STATS))}
        if out is None:
            res = {}
        else:
            res = AtcVecEnv._results(self, out, want, set(), "out must be a dict with any of grad, stats, value, scratch")
        for n in ("grad", "stats"):
            if n not in res:
                res[n] = torch.empty(want[n][1], dtype=torch.float32, device=dev)
        if "value" not in res:
            res["value"] = torch.full((R,), float("nan"), dtype=torch.float32, device=dev)
        scratch = res.pop("scratch", None)
        if scratch is None:
            scratch = torch.empty((G, words + L.PPO_VALUE_STATS), dtype=torch.float32, device=dev)
        g = _lib.AtcPpoValueGrad(float(clip), workgroups)
        o = _lib.AtcPpoValueGradOut(res["grad"].data_ptr(), res["stats"].data_ptr(), res["value"].data_ptr(), scratch.data_ptr())
        fn = self._lib.atc_ppo_value_grad
        with torch.cuda.device(dev):
            rc = fn(self.sector.handle, R_src, R, K, weights.data_ptr(), obs_rows.data_ptr(), None if traffic is None else traffic.data_ptr(), v_old.data_ptr(),
                    ret.data_ptr(), None if mask is None else mask.data_ptr(), None if index is None else index.data_ptr(), C.byref(g), C.byref(o), self._stream())
            if rc:
                _lib.check(rc)
        self._keep_ppo_value_grad = (weights, obs_rows, traffic, v_old, ret, mask, index, scratch)   # they outlive the two launches
        return res

    def adv_normalise(self, adv, mask=None, *, eps=1e-8, workgroups=0, out=None):
        """Mean, standard deviation and the normalised advantages of a collection in one call on this env's current stream (atc_adv_normalise,
        include/atc_step.h): two launches, nothing is read on the host.  adv: float32, any shape, contiguous, on this env's device; mask: uint8
        with as many elements (rollout_policy_ends' control) or None — a row whose mask is 0 takes no part and is not read.
        In float64: mean = S / n, std = sqrt(max(0, S2 - S mean) / (n - 1)) (torch.std's unbiased form; 0 with n == 1); then in float32
        out = (adv - float32(mean)) * float32(1 / (std + eps)) — ppo_policy_grad's A = (adv - adv_shift) * adv_scale word for word — and 0
        where a row takes no part.  Returns {"adv": of adv's shape, "stats": [4] (the L.ADV_STAT_* words: n, mean, scale, std)}; all zeros
        with n == 0.  out: a dict with any of "adv" (which may be the input itself: in place), "stats" and "scratch" (float64 [G, 3] with
        G = L.adv_workgroups(R, workgroups)); with all three the method allocates nothing.  workgroups: 0, or G = 1 .. L.ADV_MAX_WG — the same
        inputs and the same G give the same bits on every run."""
        torch = self.torch
        dev, f32 = self.device, (self.torch.float32,)
        need = AtcVecEnv._on_device.__get__(self)
        if not (torch.is_tensor(adv) and 1 <= adv.numel() <= 2 ** 31 - 1):
            raise ValueError("adv must be a float32 tensor of 1 .. 2^31 - 1 elements")
        R, shape = int(adv.numel()), tuple(adv.shape)
        need(adv, f32, shape, "adv")
        if mask is not None:
            need(mask, (torch.uint8,), (R,), "mask", elements=True)
        with np.errstate(over="ignore"):
            if not (np.isfinite(np.float32(eps)) and np.float32(eps) >= 0):
                raise ValueError("eps must be finite (in float32) and >= 0")
        workgroups = int(workgroups)
        if not 0 <= workgroups <= L.ADV_MAX_WG:
            raise ValueError("0 <= workgroups <= %d" % L.ADV_MAX_WG)
        G = L.adv_workgroups(R, workgroups)
        want = {"adv": (f32, shape), "stats": (f32, (L.ADV_STATS,)), "scratch": ((torch.float64,), (G, 3))}
        res = {} if out is None else AtcVecEnv._results(self, out, want, set(), "out must be a dict with any of adv, stats, scratch")
        if "adv" not in res:
            res["adv"] = torch.empty(shape, dtype=torch.float32, device=dev)
        if "stats" not in res:
            res["stats"] = torch.empty(L.ADV_STATS, dtype=torch.float32, device=dev)
        scratch = res.pop("scratch", None)
        if scratch is None:
            scratch = torch.empty((G, 3), dtype=torch.float64, device=dev)
        g = _lib.AtcAdvNorm(float(eps), workgroups)
        o = _lib.AtcAdvNormOut(res["adv"].data_ptr(), res["stats"].data_ptr(), scratch.data_ptr())
        fn = self._lib.atc_adv_normalise
        with torch.cuda.device(dev):
            rc = fn(self.sector.handle, R, adv.data_ptr(), None if mask is None else mask.data_ptr(), C.byref(g), C.byref(o), self._stream())
            if rc:
                _lib.check(rc)
        self._keep_adv_normalise = (adv, mask, scratch)      # they outlive the two launches
        return res

    def adam_step(self, tensors, *, lr, step, beta1=0.9, beta2=0.999, eps=1e-5, max_norm=0.0, out=None):
        """PPO2's optimiser step on one or two packed tensors in ONE launch on this env's current stream (atc_adam_step, include/atc_step.h):
        the gradient-norm clip over all of them, the entropy term, and torch.optim.Adam's update, in float64 with one rounding per stored word.
        tensors: a list of 1 - 2 dicts {"w", "grad", "m", "v": contiguous float32 tensors of the same 1 .. L.ADAM_MAX_WORDS elements on this
        env's device, all updated in place but grad; "grad_scale": 1.0 (vf_coef for the critic); "add": (first, count, value) or None — value is
        added to the effective gradient of words first .. first + count - 1: the entropy bonus is (policy.offsets(K)["log_std"][0], 3, -ent_coef)}.
        lr; step: the number of this update, from 1 (the bias corrections 1 - beta^step); max_norm: <= 0 or inf: no clip, else the norm over
        all tensors' effective gradients is clipped to it (clip_grad_norm_'s rule).  A norm that is not finite skips the update: w, m, v keep
        their bits.  Returns `stats` [4] (the L.ADAM_STAT_* words: norm, the coefficient applied, skipped, step); out: that tensor, and
        nothing is allocated.  No two tensors of the call may share memory (refused by the library)."""
        torch = self.torch
        f32 = (torch.float32,)
        need = AtcVecEnv._on_device.__get__(self)
        if not (isinstance(tensors, (list, tuple)) and 1 <= len(tensors) <= 2 and all(isinstance(t, dict) for t in tensors)):
            raise ValueError("tensors must be a list of 1 or 2 dicts with w, grad, m, v (and grad_scale, add)")
        arr = (_lib.AtcAdamTensor * len(tensors))()
        for k, t in enumerate(tensors):
            if not {"w", "grad", "m", "v"} <= t.keys() <= {"w", "grad", "m", "v", "grad_scale", "add"}:
                raise ValueError("tensors[%d] must be a dict with w, grad, m, v (and grad_scale, add)" % k)
            w = t["w"]
            if not (torch.is_tensor(w) and 1 <= w.numel() <= L.ADAM_MAX_WORDS):
                raise ValueError("tensors[%d]['w'] must be a float32 tensor of 1 .. %d elements" % (k, L.ADAM_MAX_WORDS))
            words = int(w.numel())
            for n in ("w", "grad", "m", "v"):
                need(t[n], f32, (words,), "tensors[%d][%r]" % (k, n), elements=True)
            first, count, value = t.get("add") or (0, 0, 0.0)
            first, count = int(first), int(count)
            if count < 0 or (count > 0 and not 0 <= first <= words - count):
                raise ValueError("tensors[%d]['add'] = (first, count, value) must lie inside the tensor" % k)
            scale = float(t.get("grad_scale", 1.0))
            with np.errstate(over="ignore"):
                if not (np.isfinite(np.float32(scale)) and np.isfinite(np.float32(value))):
                    raise ValueError("tensors[%d]: grad_scale and the added value must be finite in float32" % k)
            arr[k] = _lib.AtcAdamTensor(w.data_ptr(), t["grad"].data_ptr(), t["m"].data_ptr(), t["v"].data_ptr(), words, scale, first, count, float(value))
        step = int(step)
        if not 1 <= step <= 2 ** 31 - 1:
            raise ValueError("step must be >= 1 (the number of this update)")
        lr, beta1, beta2, eps, max_norm = float(lr), float(beta1), float(beta2), float(eps), float(max_norm)
        if not (np.isfinite(lr) and lr >= 0 and np.isfinite(eps) and eps >= 0):
            raise ValueError("lr and eps must be finite and >= 0")
        if not (0 <= beta1 < 1 and 0 <= beta2 < 1):
            raise ValueError("beta1 and beta2 must lie in [0, 1)")
        if max_norm != max_norm:
            raise ValueError("max_norm must not be a NaN (<= 0 or inf: no clip)")
        if out is None:
            out = torch.empty(L.ADAM_STATS, dtype=torch.float32, device=self.device)
        else:
            need(out, f32, (L.ADAM_STATS,), "out")
        g = _lib.AtcAdam(lr, beta1, beta2, eps, max_norm, step)
        fn = self._lib.atc_adam_step
        with torch.cuda.device(self.device):
            rc = fn(self.sector.handle, len(tensors), arr, C.byref(g), out.data_ptr(), self._stream())
            if rc:
                _lib.check(rc)
        self._keep_adam_step = [tuple(t[n] for n in ("w", "grad", "m", "v")) for t in tensors]      # they outlive the launch
        return out

    def get_attr(self, name, indices=None):
        """VecEnv.get_attr for the attributes the reference's trainer reads (learning/atc-gym-stable-baselines.py:34,36)
        and the episode counters."""
        torch = self.torch
        if name == "actions_per_timestep":
            # atc_gym.py:197 sets it on every step and reset() leaves it alone: an env that has just been (auto-)reset still
            # reports the value of its last episode's final step
            live = self.actions_taken.to(torch.float64) / self.timesteps.clamp(min=1).to(torch.float64)
            last = self.ep_actions.to(torch.float64) / self.ep_length.clamp(min=1).to(torch.float64)
            t = torch.where(self.timesteps > 0, live, last)
        elif name == "winning_ratio":  # atc_gym.py:362-363: mean of the last 10 episode outcomes
            bits = self.win_bits.to(torch.int64)
            t = sum(((bits >> k) & 1) for k in range(10)).to(torch.float64) / 10.0
        elif name in ("timesteps", "actions_taken", "total_reward", "episodes", "ep_return", "ep_length", "ep_actions"):
            t = getattr(self, name)
        else:
            raise AttributeError(name)
        vals = t.cpu().tolist()
        if indices is not None:
            vals = [vals[i] for i in indices]
        return vals

    @property
    def active_mask(self):
        """u64 mask per env (bit k = aircraft k still under control) as an int64 tensor."""
        lo = self.env[:, L.ENV_MASK_LO].to(self.torch.int64) & 0xffffffff
        hi = self.stats[:, L.STAT_MASK_HI].to(self.torch.int64) & 0xffffffff
        return lo | (hi << 32)

    # positions live on the sector's 32-bit fixed-point grid (include/atc_step.h "Aircraft positions"):
    # nm = origin + counts * 2^-k.  `x` / `y` are float64 COPIES in nautical miles; write through set_state / set_xy.
    # Speed and heading are fixed point too (ABI 18): kt = v_fix 2^-23 (unsigned counts), deg = 180 + phi_fix 2^-23; `v` / `phi`
    # are float64 copies in knots / degrees (exact), written through set_state / set_v / set_phi.
    @property
    def x(self):
        return self.ac[:, L.AC_X].to(self.torch.float64) * 2.0 ** -self.pos_k + self.pos_origin[0]

    @property
    def y(self):
        return self.ac[:, L.AC_Y].to(self.torch.float64) * 2.0 ** -self.pos_k + self.pos_origin[1]

    @property
    def v(self):
        return (self.v_fix.to(self.torch.int64) & 0xffffffff).to(self.torch.float64) * 2.0 ** -L.V_FIX_SHIFT

    @property
    def phi_counts(self):
        """exact heading counts as float64 (integer-valued): the 32-bit field, or the side record where that is saturated"""
        f = self.phi_fix
        wide = (f == L.I32_MIN) | (f == L.I32_MAX)
        return self.torch.where(wide, self.phi_wide[:, 0], f.to(self.torch.float64))

    @property
    def phi(self):
        return self.phi_counts * 2.0 ** -L.PHI_FIX_SHIFT + L.PHI_FIX_OFFSET

    def _to_fix(self, value, axis):
        from .scenario import to_fix
        return int(to_fix(float(value), self.pos_origin[axis], self.pos_k))

    @staticmethod
    def _v_counts(v):
        """knots -> speed counts as the int32 word that holds the unsigned value"""
        c = int(min(max(round(float(v) * 2.0 ** L.V_FIX_SHIFT), 0), 2 ** 32 - 1))
        return c - (1 << 32) if c >= 1 << 31 else c

    @staticmethod
    def _phi_counts(phi):
        """degrees -> (32-bit field, exact counts): the field saturates, the exact counts are clamped to +-2^52 (include/atc_step.h)"""
        P = int(min(max(round((float(phi) - L.PHI_FIX_OFFSET) * 2.0 ** L.PHI_FIX_SHIFT), -L.PHI_LIMIT), L.PHI_LIMIT))
        return min(max(P, L.I32_MIN), L.I32_MAX), P

    def _put_phi(self, field, i, col, phi):
        f, P = self._phi_counts(phi)
        field[i] = f
        if f in (L.I32_MIN, L.I32_MAX):
            self.phi_wide[i, col] = float(P)

    def set_xy(self, i, x=None, y=None):
        if x is not None:
            self.ac[i, L.AC_X] = self._to_fix(x, 0)
        if y is not None:
            self.ac[i, L.AC_Y] = self._to_fix(y, 1)

    def set_v(self, i, v):
        # The speed's rate limit is a wrapping 32-bit difference (include/atc_step.h): exact while the speed lies within 256 kt
        # of every acceptable target [100, 300] kt, i.e. inside [44, 356] kt.  The reference's constructor refuses anything outside
        # [100, 300] (model.py:22-23); a speed poked in from outside (env._airplane.v = ...) is refused beyond the format's range.
        if not 44.0 <= float(v) <= 356.0:
            raise ValueError("invalid velocity: the device's speed format holds 44 .. 356 kt (an Airplane has 100 .. 300)")
        self.v_fix[i] = self._v_counts(v)

    def set_phi(self, i, phi):
        self._put_phi(self.phi_fix, i, 0, phi)

    def set_state(self, env, slot, x, y, h, phi, v):
        i = env * self.N + slot
        self.set_xy(i, x, y)
        self.h[i] = float(h)
        self.set_phi(i, phi)
        self.set_v(i, v)

    def get_last_action(self, env, slot):
        """AtcGym.last_action (atc_gym.py:86,311) of one aircraft: [v, h, phi] targets last accepted, in kt / ft / deg."""
        i = env * self.N + slot
        rec = self.last_act[i].cpu()
        lp = int(rec[L.LA_PHI])
        if lp in (L.I32_MIN, L.I32_MAX):
            lp = float(self.phi_wide[i, 1])
        return [float(int(rec[L.LA_V]) & 0xffffffff) * 2.0 ** -L.V_FIX_SHIFT,
                float(rec[L.LA_H:L.LA_H + 2].contiguous().view(self.torch.float64)[0]),
                float(lp) * 2.0 ** -L.PHI_FIX_SHIFT + L.PHI_FIX_OFFSET]

    def set_last_action(self, env, slot, value):
        i = env * self.N + slot
        torch = self.torch
        f, P = self._phi_counts(value[2])
        rec = torch.tensor([self._v_counts(value[0]), f, 0, 0], dtype=torch.int32)
        rec[L.LA_H:L.LA_H + 2].view(torch.float64)[0] = float(value[1])
        self.last_act[i] = rec.to(self.last_act.device)
        if f in (L.I32_MIN, L.I32_MAX):
            self.phi_wide[i, 1] = float(P)

    def get_state(self, env, slot):
        i = env * self.N + slot
        return [float(t[i]) for t in (self.x, self.y, self.h, self.phi, self.v)]

    def synchronize(self):
        self.torch.cuda.synchronize(self.device)

    def close(self):
        self.sector.close()


def make_multi_launcher(envs, actions, streams, held=False):
    """One step of several INDEPENDENT sub-batch envs with a single foreign call (`atc_step_multi`): envs[i] steps with
    the device tensor actions[i] on streams[i].  Returns a no-argument callable that only launches.  With no join between
    steps the sub-batches run decoupled: the launch ramp and tail of one overlap the body of the others (bench.py
    --streams, tools/multi_stream.py)."""
    n = len(envs)
    assert n == len(actions) == len(streams) and n >= 1
    built = [e.step_call(a, q, held) for e, a, q in zip(envs, actions, streams)]
    arr = (_lib.AtcStepCall * n)(*[b[0] for b in built])
    fn, check = _lib.load().atc_step_multi, _lib.check

    def launch(_keep=(built, arr)):
        rc = fn(n, arr)
        if rc:
            check(rc)
    return launch
