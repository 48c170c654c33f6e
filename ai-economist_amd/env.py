"""Device backend: owns the arena (a torch uint8 CUDA/HIP tensor), the `aie_env` handle
and zero-copy torch views of every exported tensor.  torch is plumbing here (memory,
streams, distributed); all compute happens in the HIP kernels behind the C ABI.
"""
import ctypes as C

import numpy as np

from . import _cabi, _native

_TORCH_DTYPES = None


def _torch():
    import torch

    global _TORCH_DTYPES
    if _TORCH_DTYPES is None:
        _TORCH_DTYPES = [torch.uint8, torch.int8, torch.int16, torch.int32, torch.int32,
                         torch.float32, torch.float64]  # uint32 exposed as int32 bits
    return torch


class AieError(RuntimeError):
    pass


class DeviceBackend:
    def __init__(self, cfg, layout_planes, device=None):
        torch = _torch()
        if not torch.cuda.is_available():
            raise AieError("no HIP device visible: the batched env has no CPU fallback")
        # AIE_DEV_LIB=1: the -DAIE_DEV build with the development hooks (tools/, a few tests); never the default
        import os

        self.lib = _native.lib(dev=os.environ.get("AIE_DEV_LIB") == "1")
        self.cfg = cfg
        # names of the environment's host components (foundation.BatchedComponent), set by the environment: whole-step
        # calls and auto-reset are refused then (_refuse_with_host_components)
        self.host_components = ()
        if device is None:
            device = torch.device("cuda", torch.cuda.current_device())
        self.device = torch.device(device)
        if self.device.index is None:  # "cuda": the CURRENT device, which is where torch allocates the arena
            self.device = torch.device("cuda", torch.cuda.current_device())
        nbytes = self.lib.aie_arena_bytes(C.byref(cfg))
        if nbytes < 0:
            raise self._err(None, nbytes)
        # Small arenas are torch allocations (the caching allocator hands them out without a device call).  Large ones
        # (AIE_ARENA_VMM_MIN_MB, default 1 GiB, and up) are allocated by the library as a virtual range backed by 64 MiB
        # physical pieces: the store-bound one-step-economy launch over its 7 GB arena runs 14 % faster that way than on
        # one allocation of torch's or hipMalloc's (csrc/aie_capi.hip: aie_arena_alloc, profiles/r04_c5_alloc.json);
        # the library owns that memory until aie_destroy, `self.arena` is a view of it.
        lib_owned = int(nbytes) >= (int(os.environ.get("AIE_ARENA_VMM_MIN_MB", "1024")) << 20) and \
            os.environ.get("AIE_ARENA_PIECE_MB", "64") != "0"
        self.arena = None if lib_owned else torch.zeros(int(nbytes), dtype=torch.uint8, device=self.device)
        h = C.c_void_p()
        with torch.cuda.device(self.device):
            rc = self.lib.aie_create(C.byref(cfg), self.device.index, self.arena.data_ptr() if self.arena is not None else None,
                                     int(nbytes), C.byref(h))
        if rc != 0:
            raise self._err(None, rc)
        self.handle = h
        try:
            self._finish_init(cfg, layout_planes, lib_owned, nbytes)
        except BaseException:
            # nothing else knows the handle yet: destroy it (and a library-owned arena with it) instead of leaking it.
            # Exactly once: an owner object, once it exists, destroys the handle in its __del__ -- which may
            # run right here or later, when the last view of the arena goes -- so it is disarmed first and the one
            # aie_destroy call is this one.
            owner = getattr(self, "_arena_owner", None)
            if owner is not None:
                owner.handle = None
            self._arena_owner = None
            self.tensors = {}
            self.arena = None
            try:
                self.lib.aie_destroy(self.handle)
            finally:
                self.handle = None
            raise

    def _finish_init(self, cfg, layout_planes, lib_owned, nbytes):
        torch = _torch()
        if lib_owned:
            d0 = _cabi.AieTensorDesc()
            self.lib.aie_tensor_at(self.handle, 0, C.byref(d0))
            base = int(d0.data) - int(d0.arena_offset)

            class _Arena:
                """The library's allocation as a CUDA array (torch wraps it without copying and keeps this object alive
                for as long as any view of the arena lives): it owns the environment handle, so the memory is released
                -- aie_destroy -- when the last tensor that points into it is gone, not when the backend is closed."""
                __cuda_array_interface__ = {"shape": (int(nbytes),), "typestr": "|u1", "data": (base, False), "version": 2}

                def __init__(self, lib, handle):
                    self.lib, self.handle = lib, handle

                def __del__(self):
                    try:
                        if self.handle:
                            self.lib.aie_destroy(self.handle)
                    except Exception:
                        pass

            self._arena_owner = _Arena(self.lib, self.handle)
            self.arena = torch.as_tensor(self._arena_owner, device=self.device)
        self.E = cfg.n_envs
        self.n = cfg.n_agents
        self.descs = {}
        self.tensors = {}
        d = _cabi.AieTensorDesc()
        for i in range(self.lib.aie_num_tensors(self.handle)):
            self.lib.aie_tensor_at(self.handle, i, C.byref(d))
            name = d.name.decode()
            self.descs[name] = (d.dtype, tuple(d.shape[: d.ndim]), tuple(d.stride[: d.ndim]),
                                d.arena_offset)
            self.tensors[name] = self._view(*self.descs[name])
        stone_src, wood_src, water = [np.ascontiguousarray(p, np.uint8) for p in layout_planes]
        self._check(self.lib.aie_set_layout(self.handle, stone_src.ctypes.data,
                                            wood_src.ctypes.data, water.ctypes.data))
        self._rand_a = None
        self._rand_p = None
        # element counts the kernels index (aie_kernels.hip: decode_actions reads aa[(e*n + i) * act_a_width + s] and
        # ap[e * act_p_width + b]): checked on every call, a wrongly shaped buffer would be read out of bounds
        wa = 1 if not cfg.multi_action_mode_agents else max(1, self._n_sub_a())
        self.act_a_numel = self.E * self.n * wa
        self.act_p_numel = self.E * self._act_p_width_for(cfg)

    # ---- plumbing ----
    def _err(self, handle, rc):
        msg = self.lib.aie_last_error(handle)
        msg = msg.decode() if msg else ""
        if rc == _cabi.E_NOTFOUND:
            return KeyError(msg)
        if rc == _cabi.E_INVALID:
            return ValueError(msg)
        if rc == _cabi.E_UNSUPPORTED:
            return NotImplementedError(msg)
        return AieError("aie error %d: %s" % (rc, msg))

    def _check(self, rc):
        if rc != 0:
            raise self._err(self.handle, rc)

    def _view(self, dtype, shape, stride, offset):
        torch = _torch()
        tdt = _TORCH_DTYPES[dtype]
        es = torch.empty(0, dtype=tdt).element_size()
        base = self.arena[offset:]
        usable = (base.numel() // es) * es
        typed = base[:usable].view(tdt)
        assert all(s % es == 0 for s in stride)
        return torch.as_strided(typed, shape, tuple(s // es for s in stride))

    def _stream(self):
        return C.c_void_p(_torch().cuda.current_stream(self.device).cuda_stream)

    def _ptr(self, t, dtype, what, numel=None):
        torch = _torch()
        if t is None:
            return None
        if not isinstance(t, torch.Tensor):
            t = torch.as_tensor(np.asarray(t), device=self.device)
        if numel is not None and t.numel() != numel:
            raise ValueError("%s has %d elements (shape %s), the environment needs %d: actions_a is int32 "
                             "[n_envs, n_agents(, n_subspaces)], actions_p int32 [n_envs, planner subspaces], env_mask "
                             "uint8 [n_envs]" % (what, t.numel(), tuple(t.shape), numel))
        if t.device != self.device:
            t = t.to(self.device)
        if t.dtype != dtype:
            t = t.to(dtype)
        t = t.contiguous()
        self._keep = getattr(self, "_keep", [])
        self._keep = self._keep[-8:] + [t]  # keep alive until the stream has consumed it
        return C.c_void_p(t.data_ptr())

    # ---- API ----
    def seed(self, base_seed):
        """Replica e gets the stream of seed base_seed + e: np.random.seed(base_seed + e) (rng_mode "numpy"), or the
        counter stream keyed by base_seed + e (rng_mode "fast": aie_seed_fast, 48 bits of the seed are used)."""
        if self.cfg.rng_mode == _cabi.RNG_FAST:
            self._check(self.lib.aie_seed_fast(self.handle, C.c_uint64(base_seed & 0xFFFFFFFFFFFFFFFF), C.c_int64(0), self._stream()))
        else:
            self._check(self.lib.aie_seed(self.handle, C.c_uint32(base_seed & 0xFFFFFFFF), self._stream()))

    def set_rng_state(self, keys, pos):
        words = _cabi.RNG_FAST_STATE_WORDS if self.cfg.rng_mode == _cabi.RNG_FAST else _cabi.MT_N
        keys = np.ascontiguousarray(keys, np.uint32).reshape(self.E, words)
        pos = np.ascontiguousarray(pos, np.int32).reshape(self.E)
        self._check(self.lib.aie_set_rng_state(self.handle, keys.ctypes.data, pos.ctypes.data))

    def reset(self, env_mask=None):
        torch = _torch()
        m = self._ptr(env_mask, torch.uint8, "env_mask", self.E)
        self._check(self.lib.aie_reset(self.handle, m, self._stream()))

    def _refuse_with_host_components(self, what):
        """An environment with host components (foundation.BatchedComponent) marks its backend: a whole step or an
        auto-reset inside the step would run without the components' hooks, so those calls raise instead."""
        if self.host_components:
            raise NotImplementedError(
                "%s: this environment has host components (%s); a whole-step launch or an auto-reset would skip their "
                "hooks -- step and reset it through env.step / env.reset" % (what, ", ".join(self.host_components)))

    def step(self, actions_a=None, actions_p=None):
        self._refuse_with_host_components("Backend.step")
        torch = _torch()
        a = self._ptr(actions_a, torch.int32, "actions_a", self.act_a_numel)
        p = self._ptr(actions_p, torch.int32, "actions_p", self.act_p_numel)
        self._check(self.lib.aie_step(self.handle, a, p, self._stream()))

    def step_range(self, actions_a, actions_p, comp_lo, comp_hi, phases, mask=None):
        """aie_step_range: the built-in components [comp_lo, comp_hi) and the named parts of a step (_cabi.STEP_HEAD /
        STEP_TAIL / STEP_OBSERVE, or the end of a step in its parts STEP_REGEN / STEP_EMIT / STEP_CLOSE) -- what
        foundation.BatchedComponent hooks and scenario hooks run between.  mask: uint8 [E] device tensor
        of the replicas the launch touches (a masked reset's follow-up launches), None = all."""
        torch = _torch()
        a = self._ptr(actions_a, torch.int32, "actions_a", self.act_a_numel)
        p = self._ptr(actions_p, torch.int32, "actions_p", self.act_p_numel)
        m = self._ptr(mask, torch.uint8, "env_mask", self.E)
        self._check(self.lib.aie_step_range(self.handle, a, p, int(comp_lo), int(comp_hi), int(phases), self._stream(), m))

    def set_reward_log(self, n_slots):
        """Allocates a reward log of `n_slots` step slots, f32 [n_slots, E, n_agents + 2] = (agent rewards,
        planner reward, done), and makes every following step fill the next slot (slot 0 first, wrapping).
        n_slots = 0 switches it off.  Returns the log tensor (or None)."""
        torch = _torch()
        if not n_slots:
            self._check(self.lib.aie_set_reward_log(self.handle, None, 0))
            self.reward_log = None
            return None
        self.reward_log = torch.zeros((int(n_slots), self.E, self.n + 2), dtype=torch.float32, device=self.device)
        self._check(self.lib.aie_set_reward_log(self.handle, C.c_void_p(self.reward_log.data_ptr()), int(n_slots)))
        return self.reward_log

    def rewind_reward_log(self):
        """The next step fills slot 0 of the current reward log again."""
        if self.reward_log is not None:
            self._check(self.lib.aie_set_reward_log(self.handle, C.c_void_p(self.reward_log.data_ptr()),
                                                    int(self.reward_log.shape[0])))

    def set_auto_reset(self, on=True):
        """Replicas restart inside / right behind the step that ends their episode (include/aie.h:
        aie_set_auto_reset): `done` and the rewards are the terminal step's, state and observations the new episode's."""
        if on:
            self._refuse_with_host_components("Backend.set_auto_reset(True)")
        self._check(self.lib.aie_set_auto_reset(self.handle, 1 if on else 0))

    def set_dense_log_active(self, on=True):
        """Dense-log replicas record event rows (and run the full-featured kernel) only while an episode is being
        logged (include/aie.h: aie_set_dense_log_active); otherwise they step with the rest of the batch."""
        self._check(self.lib.aie_set_dense_log_active(self.handle, 1 if on else 0))

    def step_sample_next(self, actions_a, actions_p, seed, env_offset=0, next_slot=1, masked=False):
        """One launch: step with (actions_a, actions_p) and fill the action buffers of `next_slot`
        with the uniform random policy's next draw (same values as sample_random_actions; masked=True, COVID only:
        as sample_masked_actions, from the masks this step writes)."""
        self._refuse_with_host_components("Backend.step_sample_next")
        torch = _torch()
        a = self._ptr(actions_a, torch.int32, "actions_a", self.act_a_numel)
        p = self._ptr(actions_p, torch.int32, "actions_p", self.act_p_numel)
        na, np_ = self._action_buffers(next_slot)
        fn = self.lib.aie_step_sample_next_masked if masked else self.lib.aie_step_sample_next
        self._check(fn(
            self.handle, a, p, C.c_uint64(seed), C.c_int64(env_offset),
            C.c_void_p(na.data_ptr()), C.c_void_p(np_.data_ptr()), self._stream()))
        return na, np_

    def arena_info(self):
        """{"bytes", "allocator": "caller" (a torch tensor) | "hipMalloc" | "vmm", "piece_mib"} -- aie_arena_info."""
        b, a, pc = C.c_int64(), C.c_int32(), C.c_int64()
        self._check(self.lib.aie_arena_info(self.handle, C.byref(b), C.byref(a), C.byref(pc)))
        name = _cabi.ARENA_ALLOCATORS[a.value]
        return {"bytes": int(b.value), "allocator": "torch" if name == "caller" else name, "piece_mib": int(pc.value) >> 20}

    def specialize(self, required=False):
        """aie_specialize: kernels compiled for this configuration at run time (hiprtc, cached).  Returns True when the
        environment now runs on specialised kernels; False (or, with required=True, an exception) when that is not
        possible here -- the generic kernel keeps running, with identical results."""
        rc = self.lib.aie_specialize(self.handle)
        if rc != 0 and required:
            raise self._err(self.handle, rc)
        return rc == 0

    def sample_masked_actions(self, seed, env_offset=0, slot=0):
        """Like sample_random_actions, but every sub-action is drawn uniformly among the
        entries the current `action_mask` observations allow."""
        self.sample_random_actions  # noqa: B018  (buffers are shared)
        a, p = self._action_buffers(slot)
        self._check(self.lib.aie_sample_masked_actions(
            self.handle, C.c_uint64(seed), C.c_int64(env_offset),
            C.c_void_p(a.data_ptr()), C.c_void_p(p.data_ptr()), self._stream()))
        return a, p

    def sample_policy_actions(self, logits_a, logits_p, seed, env_offset=0, slot=0, out=None, logp=False):
        """Categorical sampling from the caller's policy logits under the current action masks (aie_sample_policy_actions:
        inverse-CDF sampling in float32 -- weights exp(logit - max) of the allowed entries, prefix sums in a fixed order,
        one counter-hash uniform per slot -- in one launch, replayable from a captured graph).  logits_a: float32
        [E, n, MA] in the layout of the agents' flattened action mask (COVID: [E, n, 1 + levels]), logits_p: float32
        [E, MP]; either may be None.
        Returns the action buffers (int32 [E, n, width], [E, width_p]) -- `out=(a, p)` to fill the caller's own.
        logp=True (aie_sample_policy_actions_logp: the same picks, the same launch count): returns (a, p, logp_a, logp_p),
        float32 tensors of the actions' shapes with log pi(a|s) of every pick under the masks it was drawn under --
        `out=(a, p, logp_a, logp_p)` to fill the caller's own.  The buffers of an actor class whose logits are None are
        left alone."""
        torch = _torch()
        if out is not None:
            a, p = out[0], out[1]
        else:
            a, p = self._action_buffers(slot)
        la = lp = None
        if logits_a is not None:
            per_agent = self.tensors["obs_a_action_mask"].numel() // (self.E * self.n)
            la = self._ptr(logits_a, torch.float32, "logits_a", self.E * self.n * per_agent)
        if logits_p is not None:
            lp = self._ptr(logits_p, torch.float32, "logits_p", self.tensors["obs_p_action_mask"].numel())
        pa = C.c_void_p(a.data_ptr()) if logits_a is not None else None
        pp = C.c_void_p(p.data_ptr()) if logits_p is not None else None
        if not logp:
            self._check(self.lib.aie_sample_policy_actions(
                self.handle, la, lp, C.c_uint64(seed), C.c_int64(env_offset), pa, pp, self._stream()))
            return a, p
        if out is not None and len(out) == 4:
            ga, gp = out[2], out[3]
        else:
            ga, gp = self._logp_buffers(slot)
        for t, like, what in ((ga, a, "logp_a"), (gp, p, "logp_p")):
            if t.dtype != torch.float32 or t.numel() != like.numel() or not t.is_contiguous() or t.device != self.device:
                raise ValueError("%s: a contiguous float32 device tensor of the action buffer's %d elements" % (what, like.numel()))
        self._check(self.lib.aie_sample_policy_actions_logp(
            self.handle, la, lp, C.c_uint64(seed), C.c_int64(env_offset), pa, pp,
            C.c_void_p(ga.data_ptr()) if logits_a is not None else None,
            C.c_void_p(gp.data_ptr()) if logits_p is not None else None, self._stream()))
        return a, p, ga, gp

    def _logp_buffers(self, slot):
        torch = _torch()
        if getattr(self, "_logp_bufs", None) is None:
            a, p = self._action_buffers(0)
            self._logp_bufs = [(torch.zeros(a.shape, dtype=torch.float32, device=self.device),
                                torch.zeros(p.shape, dtype=torch.float32, device=self.device)) for _ in range(2)]
        return self._logp_bufs[slot]

    def action_masks(self, out=None):
        """A snapshot (masks_a, masks_p) of the current action masks in the LOGITS' layout -- float32 [E, n, MA]
        (COVID: [E, n, 1 + levels], a transposing copy of the arena's collated rows) and [E, MP] -- to store in a
        trajectory beside the actions and evaluate later (policy_evaluate / rollout.masked_logp_entropy).  Plain device
        copies on the current stream (capturable); `out=(masks_a, masks_p)` to fill the caller's own."""
        torch = _torch()
        ma, mp = self.tensors["obs_a_action_mask"], self.tensors["obs_p_action_mask"]
        if int(self.cfg.scenario) == _cabi.SCN_COVID:
            ma = ma.transpose(1, 2)  # [E, 1 + levels, n] -> [E, n, 1 + levels]
        if out is None:
            out = (torch.empty(ma.shape, dtype=torch.float32, device=self.device),
                   torch.empty(mp.shape, dtype=torch.float32, device=self.device))
        out[0].view(ma.shape).copy_(ma)
        out[1].view(mp.shape).copy_(mp)
        return out[0], out[1]

    def _policy_eval_operands(self, logits_a, logits_p, masks_a, masks_p, actions_a, actions_p):
        """Contiguous device operands of aie_policy_evaluate / _backward and the batch size B they agree on."""
        torch = _torch()
        per_a = self.tensors["obs_a_action_mask"].numel() // self.E
        per_p = self.tensors["obs_p_action_mask"].numel() // self.E
        aa, ap = self._action_buffers(0)
        act_a, act_p = aa.numel() // self.E, ap.numel() // self.E

        def dev(t, dtype):
            if t is None:
                return None
            if not isinstance(t, torch.Tensor):
                t = torch.as_tensor(np.asarray(t))
            return t.to(device=self.device, dtype=dtype).contiguous()

        ops = dict(la=dev(logits_a, torch.float32), lp=dev(logits_p, torch.float32), ma=dev(masks_a, torch.float32),
                   mp=dev(masks_p, torch.float32), aa=dev(actions_a, torch.int32), ap=dev(actions_p, torch.int32))
        per = dict(la=per_a, lp=per_p, ma=per_a, mp=per_p, aa=act_a, ap=act_p)
        Bs = set()
        for k, t in ops.items():
            if t is not None:
                if t.numel() == 0 or t.numel() % per[k]:
                    raise ValueError("policy evaluation: operand %r has %d elements, not a multiple of the %d per batch element"
                                     % (k, t.numel(), per[k]))
                Bs.add(t.numel() // per[k])
        if len(Bs) != 1:
            raise ValueError("policy evaluation: the operands disagree on the batch size (%s)" % sorted(Bs))
        return ops, Bs.pop(), (act_a, act_p, per_a, per_p)

    def policy_evaluate(self, logits_a, logits_p, masks_a, masks_p, actions_a, actions_p, entropy=True):
        """aie_policy_evaluate: (logp_a, logp_p, entropy_a, entropy_p) of stored actions under stored masks for the given
        logits, B batch elements (any B: the operands' leading extent(s); with masks None -- the arena's current masks
        -- B = E).  Layouts as sample_policy_actions / action_masks; either actor class may be None (its outputs are
        None).  One launch on the current stream."""
        torch = _torch()
        ops, B, (act_a, act_p, _, _) = self._policy_eval_operands(logits_a, logits_p, masks_a, masks_p, actions_a, actions_p)
        f = dict(dtype=torch.float32, device=self.device)
        sa, sp = ((B,) + tuple(t.shape[1:]) for t in self._action_buffers(0))
        out = [torch.empty(sa, **f) if ops["la"] is not None and ops["aa"] is not None else None,
               torch.empty(sp, **f) if ops["lp"] is not None and ops["ap"] is not None else None,
               torch.empty(sa, **f) if ops["la"] is not None and entropy else None,
               torch.empty(sp, **f) if ops["lp"] is not None and entropy else None]
        ptr = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None  # noqa: E731
        self._check(self.lib.aie_policy_evaluate(
            self.handle, C.c_int64(B), ptr(ops["la"]), ptr(ops["lp"]), ptr(ops["ma"]), ptr(ops["mp"]), ptr(ops["aa"]), ptr(ops["ap"]),
            ptr(out[0]), ptr(out[1]), ptr(out[2]), ptr(out[3]), self._stream()))
        return tuple(out)

    def policy_evaluate_backward(self, logits_a, logits_p, masks_a, masks_p, actions_a, actions_p,
                                 g_logp_a=None, g_logp_p=None, g_entropy_a=None, g_entropy_p=None):
        """aie_policy_evaluate_backward: (grad_logits_a, grad_logits_p), the logits' shapes, of
        sum(g_logp * logp + g_entropy * entropy); a None gradient counts as zeros.  One launch on the current stream."""
        torch = _torch()
        ops, B, (act_a, act_p, _, _) = self._policy_eval_operands(logits_a, logits_p, masks_a, masks_p, actions_a, actions_p)
        gs = []
        for g, per, what in ((g_logp_a, act_a, "g_logp_a"), (g_logp_p, act_p, "g_logp_p"), (g_entropy_a, act_a, "g_entropy_a"),
                             (g_entropy_p, act_p, "g_entropy_p")):
            if g is not None:
                g = g.to(device=self.device, dtype=torch.float32).contiguous()
                if g.numel() != B * per:
                    raise ValueError("%s has %d elements, the batch needs %d" % (what, g.numel(), B * per))
            gs.append(g)
        grad_a = torch.empty_like(ops["la"]) if ops["la"] is not None else None
        grad_p = torch.empty_like(ops["lp"]) if ops["lp"] is not None else None
        ptr = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None  # noqa: E731
        self._check(self.lib.aie_policy_evaluate_backward(
            self.handle, C.c_int64(B), ptr(ops["la"]), ptr(ops["lp"]), ptr(ops["ma"]), ptr(ops["mp"]), ptr(ops["aa"]), ptr(ops["ap"]),
            ptr(gs[0]), ptr(gs[1]), ptr(gs[2]), ptr(gs[3]), ptr(grad_a), ptr(grad_p), self._stream()))
        return grad_a, grad_p

    def trajectory_segment(self, src, dst, transpose_rows=0):
        """One aie_traj_segment: `src`, a device tensor whose dimension 0 is the replica ([E, ...], each replica's block
        contiguous; the replica stride may be anything -- an arena tensor's, a record field's), stored into `dst`
        ([n_slots, E, ...] contiguous, same dtype, same bytes per replica).  transpose_rows > 1: the replica's block is
        [transpose_rows][cols] 4-byte elements and is stored as [cols][transpose_rows]."""
        if src.shape[0] != self.E or dst.dim() < 2 or dst.shape[1] != self.E or src.dtype != dst.dtype:
            raise ValueError("trajectory segment: src [E, ...] and dst [n_slots, E, ...] of one dtype")
        if not dst.is_contiguous() or not src[0].is_contiguous():
            raise ValueError("trajectory segment: dst and each replica's block of src must be contiguous")
        nbytes = src[0].numel() * src.element_size()
        if nbytes != dst[0, 0].numel() * dst.element_size():
            raise ValueError("trajectory segment: %d bytes per replica in src, %d in dst"
                             % (nbytes, dst[0, 0].numel() * dst.element_size()))
        stride = (src.stride(0) if self.E > 1 else src[0].numel()) * src.element_size()
        return _cabi.AieTrajSegment(src.data_ptr(), dst.data_ptr(), stride, nbytes, int(transpose_rows)), (src, dst)

    def trajectory_store(self, segments, n_slots, slot_counters):
        """aie_trajectory_store: every segment's block of replica e goes to ring slot slot_counters[e] of its destination,
        then the counter advances modulo n_slots -- one launch on the current stream, capturable (the slot index lives on
        the device).  segments: what trajectory_segment returns (or bare _cabi.AieTrajSegment), at most
        _cabi.TRAJ_MAX_SEGMENTS; slot_counters: int32 [E] device tensor, zeroed by the caller."""
        torch = _torch()
        segs = [s[0] if isinstance(s, tuple) else s for s in segments]
        if (slot_counters.dtype != torch.int32 or slot_counters.numel() != self.E or not slot_counters.is_contiguous()
                or slot_counters.device != self.device):
            raise ValueError("slot_counters: a contiguous int32 device tensor of %d elements" % self.E)
        arr = (_cabi.AieTrajSegment * max(1, len(segs)))(*segs)
        self._check(self.lib.aie_trajectory_store(self.handle, arr, len(segs), int(n_slots),
                                                  C.c_void_p(slot_counters.data_ptr()), self._stream()))

    def gae(self, T, log, values_a, values_p, gamma, lam, first_slot=0, advantages=True, returns=True, out=None):
        """aie_gae: (adv_a, adv_p, ret_a, ret_p) of T steps from a reward log (float32 [n_slots, E, n + 2], time t in slot
        (first_slot + t) % n_slots) and the values (float32 [T + 1, E, n] / [T + 1, E], row T the bootstrap; either may be
        None).  One launch on the current stream.  out=(adv_a, adv_p, ret_a, ret_p) to fill the caller's own."""
        torch = _torch()
        T = int(T)
        f = dict(dtype=torch.float32, device=self.device)
        if log.dtype != torch.float32 or not log.is_contiguous() or log.device != self.device or log.dim() != 3 \
                or tuple(log.shape[1:]) != (self.E, self.n + 2):
            raise ValueError("gae: the log is a contiguous float32 device tensor [n_slots, %d, %d]" % (self.E, self.n + 2))
        for v, per, what in ((values_a, self.E * self.n, "values_a"), (values_p, self.E, "values_p")):
            if v is not None and (v.dtype != torch.float32 or not v.is_contiguous() or v.device != self.device
                                  or v.numel() != (T + 1) * per):
                raise ValueError("gae: %s is a contiguous float32 device tensor of (T + 1) x %d elements" % (what, per))
        if out is None:
            sa, sp = (T, self.E, self.n), (T, self.E)
            out = [torch.empty(sa, **f) if values_a is not None and advantages else None,
                   torch.empty(sp, **f) if values_p is not None and advantages else None,
                   torch.empty(sa, **f) if values_a is not None and returns else None,
                   torch.empty(sp, **f) if values_p is not None and returns else None]
        else:
            for o, per, what in zip(out, (self.E * self.n, self.E) * 2, ("adv_a", "adv_p", "ret_a", "ret_p")):
                if o is not None and (o.dtype != torch.float32 or not o.is_contiguous() or o.device != self.device
                                      or o.numel() != T * per):
                    raise ValueError("gae: %s is a contiguous float32 device tensor of T x %d elements" % (what, per))
        ptr = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None  # noqa: E731
        self._check(self.lib.aie_gae(self.handle, T, ptr(log), int(log.shape[0]), int(first_slot), ptr(values_a), ptr(values_p),
                                     C.c_float(gamma), C.c_float(lam), ptr(out[0]), ptr(out[1]), ptr(out[2]), ptr(out[3]),
                                     self._stream()))
        return tuple(out)

    def ppo_loss(self, logits_a, logits_p, values_a, values_p, batch, index=None, clip=0.3, vf_clip=50.0, vf_coef=0.05,
                 ent_coef=0.025, coeffs_p=None, adv_moments=None, out=None):
        """aie_ppo_loss: the PPO loss of both actor classes with its gradients, two launches on the current stream.
        logits_a [B, n, MA] / logits_p [B, MP] and values_a [B, n] / values_p [B] are the networks' outputs for B batch
        elements (either class None: left out; values None: no value term).  `batch` holds the STORED operands as
        contiguous device tensors of R rows -- masks_a / masks_p (float32, the logits' layout), actions_* (int32),
        logp_old_*, adv_*, values_old_*, returns_* (float32; Trajectory.ppo_batch() makes the dict) -- read at row index[b]
        (index: int32 [B] on the device) or, with index None, at row b (R == B): a minibatch is an index, nothing is
        copied and nothing is converted (a tensor of another dtype, device or layout is an error).
        clip, vf_clip, vf_coef, ent_coef: the agents' coefficients, and the planner's unless coeffs_p (a dict of any of
        them) says otherwise.  adv_moments: None or (moments_a, moments_p), each None or a float32 device tensor
        {mean, rstd}: the advantage enters as (adv - mean) * rstd.
        Returns ((stats_a, grad_logits_a, grad_values_a), (stats_p, grad_logits_p, grad_values_p)); a class that is left
        out is None, grad_values is None without values.  stats: float32 [_cabi.PPO_N_STATS] (include/aie.h); the
        gradients are those of stats[0].  Only the two gradients, the statistics and (once per backend, 1 MiB: calls of
        one backend share it and must not run at the same time on two streams) the workspace are allocated -- out=((stats_a, grad_logits_a, grad_values_a), (stats_p, ...)) to fill the caller's own instead."""
        torch = _torch()
        per_a = self.tensors["obs_a_action_mask"].numel() // self.E
        per_p = self.tensors["obs_p_action_mask"].numel() // self.E
        aa, ap = self._action_buffers(0)
        act_a, act_p = aa.numel() // self.E, ap.numel() // self.E
        f = dict(dtype=torch.float32, device=self.device)

        def net(t, per, what):  # a network output: made contiguous float32 here if it is not
            if t is None:
                return None
            t = t.detach().to(**f).contiguous()
            if t.numel() == 0 or t.numel() % per:
                raise ValueError("ppo_loss: %s has %d elements, not a multiple of the %d per batch element" % (what, t.numel(), per))
            return t

        def stored(name, dtype, per):  # a stored operand: used where it lies
            t = batch.get(name)
            if t is None:
                raise ValueError("ppo_loss: the batch has no %r" % name)
            if (not isinstance(t, torch.Tensor) or t.dtype != dtype or t.device != self.device or not t.is_contiguous()
                    or t.numel() == 0 or t.numel() % per):
                raise ValueError("ppo_loss: %s must be a contiguous %s device tensor of R x %d elements" % (name, dtype, per))
            return t

        la, lp = net(logits_a, per_a, "logits_a"), net(logits_p, per_p, "logits_p")
        if la is None and lp is None:
            raise ValueError("ppo_loss: no actor class")
        va = net(values_a, self.n, "values_a") if la is not None else None
        vp = net(values_p, 1, "values_p") if lp is not None else None
        Bs = {t.numel() // per for t, per in ((la, per_a), (lp, per_p), (va, self.n), (vp, 1)) if t is not None}
        if len(Bs) != 1:
            raise ValueError("ppo_loss: logits and values disagree on the batch size (%s)" % sorted(Bs))
        B = Bs.pop()
        if index is not None and (index.dtype != torch.int32 or index.device != self.device or not index.is_contiguous()
                                  or index.numel() != B):
            raise ValueError("ppo_loss: index must be a contiguous int32 device tensor of B = %d elements" % B)
        mom = adv_moments if adv_moments is not None else (None, None)
        coef_a = dict(clip=clip, vf_clip=vf_clip, vf_coef=vf_coef, ent_coef=ent_coef)
        coef_p = dict(coef_a, **(coeffs_p or {}))
        ptr = lambda t: t.data_ptr() if t is not None else None  # noqa: E731
        classes, outs, keep, Rs = [], [], [], set()
        for who, lg, val, per, act, actors, co, mo in (("a", la, va, per_a, act_a, self.n, coef_a, mom[0]),
                                                       ("p", lp, vp, per_p, act_p, 1, coef_p, mom[1])):
            if lg is None:
                classes.append(None)
                outs.append(None)
                continue
            ops = dict(masks=stored("masks_" + who, torch.float32, per), actions=stored("actions_" + who, torch.int32, act),
                       logp_old=stored("logp_old_" + who, torch.float32, act), adv=stored("adv_" + who, torch.float32, actors))
            pers = dict(masks=per, actions=act, logp_old=act, adv=actors, values_old=actors, returns=actors)
            if val is not None:
                ops["values_old"] = stored("values_old_" + who, torch.float32, actors)
                ops["returns"] = stored("returns_" + who, torch.float32, actors)
            Rs |= {t.numel() // pers[k] for k, t in ops.items()}
            if mo is not None and (mo.dtype != torch.float32 or mo.device != self.device or not mo.is_contiguous() or mo.numel() != 2):
                raise ValueError("ppo_loss: adv_moments are float32 device tensors {mean, rstd}")
            if out is not None:
                stats, grad, grad_v = out[who == "p"]
                for t, like, what in ((stats, None, "stats"), (grad, lg, "grad_logits"), (grad_v, val, "grad_values")):
                    numel = _cabi.PPO_N_STATS if like is None else like.numel()
                    if (t is None) != (what == "grad_values" and val is None) or (
                            t is not None and (t.dtype != torch.float32 or t.device != self.device or not t.is_contiguous()
                                               or t.numel() != numel)):
                        raise ValueError("ppo_loss: out's %s_%s must be a contiguous float32 device tensor of %d elements (None "
                                         "for grad_values without values)" % (what, who, numel))
            else:
                stats = torch.empty(_cabi.PPO_N_STATS, **f)
                grad = torch.empty_like(lg)
                grad_v = torch.empty_like(val) if val is not None else None
            c = _cabi.AiePpoClass(logits=ptr(lg), values=ptr(val), masks=ptr(ops["masks"]), actions=ptr(ops["actions"]),
                                  logp_old=ptr(ops["logp_old"]), adv=ptr(ops["adv"]), values_old=ptr(ops.get("values_old")),
                                  returns=ptr(ops.get("returns")), adv_moments=ptr(mo), grad_logits=ptr(grad),
                                  grad_values=ptr(grad_v), stats=ptr(stats), clip=co["clip"], vf_clip=co["vf_clip"],
                                  vf_coef=co["vf_coef"], ent_coef=co["ent_coef"])
            classes.append(c)
            outs.append((stats, grad, grad_v))
            keep.append(ops)
        if len(Rs) != 1 or (index is None and Rs != {B}):
            raise ValueError("ppo_loss: the stored operands have %s rows; all must agree, and without an index equal B = %d"
                             % (sorted(Rs), B))
        # the workspace: the largest any B needs (1 MiB), allocated once per backend and never replaced -- a captured call
        # keeps its pointer.  Calls of one backend share it: they must not overlap (two streams: two backends' worth of
        # workspace through the C ABI)
        ws = getattr(self, "_ppo_ws", None)
        if ws is None:
            ws = self._ppo_ws = torch.empty(_cabi.PPO_MAX_WAVES * 16, dtype=torch.float64, device=self.device)
        ref = lambda c: C.byref(c) if c is not None else None  # noqa: E731
        self._check(self.lib.aie_ppo_loss(self.handle, C.c_int64(B), ref(classes[0]), ref(classes[1]),
                                          C.c_void_p(index.data_ptr()) if index is not None else None,
                                          C.c_void_p(ws.data_ptr()), C.c_int64(ws.numel() * 8), self._stream()))
        return outs[0], outs[1]

    def _mlp_operands(self, fn, who, x, w, per):
        """The checks policy_mlp_forward and policy_mlp_backward share for one class -> (x as [rows, F], x_ld, the dict of its
        weight tensors w1 .. bv, F, H, M)."""
        torch = _torch()
        get = w.get if hasattr(w, "get") else lambda k, w=w: getattr(w, k, None)  # noqa: E731
        if x.dim() == 3:  # [B, n, F] with one row stride throughout: a view, never a copy
            if x.shape[0] > 1 and x.stride(0) != x.shape[1] * x.stride(1):
                raise ValueError("%s: x_%s [B, n, F] needs one row stride throughout (strides %s)" % (fn, who, tuple(x.stride())))
            x = x.as_strided((x.shape[0] * x.shape[1], x.shape[2]), (x.stride(1), x.stride(2)), x.storage_offset())
        if x.dim() != 2 or x.dtype != torch.float32 or x.device != self.device or (x.shape[1] > 1 and x.stride(1) != 1) \
                or x.shape[0] == 0 or x.shape[0] % per:
            raise ValueError("%s: x_%s is a float32 device tensor [B x %d, F] with contiguous rows" % (fn, who, per))
        rows, F = int(x.shape[0]), int(x.shape[1])
        x_ld = int(x.stride(0)) if rows > 1 else F
        t = {k: get(k) for k in ("w1", "b1", "w2", "b2", "w3", "b3", "wv", "bv")}
        H = int(t["w1"].shape[-1]) if t["w1"] is not None and t["w1"].dim() == 2 else 0
        M = int(t["w3"].shape[-1]) if t["w3"] is not None and t["w3"].dim() == 2 else 0
        for k, shape in (("w1", (F, H)), ("b1", (H,)), ("w2", (H, H)), ("b2", (H,)), ("w3", (H, M)), ("b3", (M,)),
                         ("wv", (H,)), ("bv", (1,))):
            v = t[k]
            if v is None and k in ("wv", "bv"):
                continue
            if (v is None or v.dtype != torch.float32 or v.device != self.device or not v.is_contiguous()
                    or v.numel() != int(np.prod(shape)) or (v.dim() == 2 and k != "wv" and tuple(v.shape) != shape)):
                raise ValueError("%s: weights_%s[%r] must be a contiguous float32 device tensor of shape %s" % (fn, who, k, shape))
        if (t["wv"] is None) != (t["bv"] is None):
            raise ValueError("%s: weights_%s needs wv and bv together" % (fn, who))
        return x, x_ld, t, F, H, M

    def policy_mlp_forward(self, x_a, x_p, weights_a, weights_p, out=None):
        """aie_policy_mlp_forward: both classes' policy network -- x -> relu -> H -> relu -> H -> logits (+ value) -- in ONE
        launch on the current stream.  x_a [B * n, F_a] (or [B, n, F_a]) and x_p [B, F_p]: float32 device tensors whose rows
        are contiguous (any row stride: an arena tensor, a sliced view); a class whose x is None is left out.  weights_*:
        a mapping (or rollout.mlp_weights) with float32 device tensors w1 [F, H], b1 [H], w2 [H, H], b2 [H], w3 [H, M],
        b3 [M], contiguous, and optionally wv [H] (or [H, 1]) with bv [1]: the value column.  The library reads them where
        they lie at every launch: update them in place and the next launch, or graph replay, sees the new values.
        Returns (logits_a [rows, M_a], logits_p [B, M_p], value_a [rows], value_p [B]) -- None for a class left out and for a
        value without wv; out=(logits_a, logits_p, value_a, value_p) fills the caller's contiguous float32 tensors instead
        (nothing is allocated).  The arithmetic contract (one ascending fmaf chain per output) is include/aie.h's."""
        torch = _torch()
        f = dict(dtype=torch.float32, device=self.device)
        out = tuple(out) if out is not None else (None,) * 4
        classes, res, Bs = [], [], set()
        for who, x, w, per, o_l, o_v in (("a", x_a, weights_a, self.n, out[0], out[2]), ("p", x_p, weights_p, 1, out[1], out[3])):
            if x is None:
                classes.append(None)
                res.append((None, None))
                continue
            x, x_ld, t, F, H, M = self._mlp_operands("policy_mlp_forward", who, x, w, per)
            rows = int(x.shape[0])
            has_v = t["wv"] is not None
            for o, numel, what in ((o_l, rows * M, "logits"), (o_v, rows, "value")):
                if o is not None and (o.dtype != torch.float32 or o.device != self.device or not o.is_contiguous() or o.numel() != numel):
                    raise ValueError("policy_mlp_forward: out's %s_%s must be a contiguous float32 device tensor of %d elements"
                                     % (what, who, numel))
            logits = o_l if o_l is not None else torch.empty((rows, M), **f)
            value = (o_v if o_v is not None else torch.empty((rows,), **f)) if has_v else None
            ptr = lambda v: v.data_ptr() if v is not None else None  # noqa: E731
            classes.append(_cabi.AieMlpClass(x=x.data_ptr(), x_ld=x_ld, w1=ptr(t["w1"]), b1=ptr(t["b1"]), w2=ptr(t["w2"]),
                                             b2=ptr(t["b2"]), w3=ptr(t["w3"]), b3=ptr(t["b3"]), wv=ptr(t["wv"]), bv=ptr(t["bv"]),
                                             logits=logits.data_ptr(), values=ptr(value), F=F, H=H, M=M))
            res.append((logits, value))
            Bs.add(rows // per)
        if not Bs:
            raise ValueError("policy_mlp_forward: no actor class")
        if len(Bs) != 1:
            raise ValueError("policy_mlp_forward: the classes disagree on the batch size (%s)" % sorted(Bs))
        ref = lambda c: C.byref(c) if c is not None else None  # noqa: E731
        self._check(self.lib.aie_policy_mlp_forward(self.handle, C.c_int64(Bs.pop()), ref(classes[0]), ref(classes[1]),
                                                    self._stream()))
        return res[0][0], res[1][0], res[0][1], res[1][1]

    def policy_mlp_backward(self, x_a, x_p, weights_a, weights_p, g_logits_a, g_logits_p, g_values_a=None, g_values_p=None,
                            out=None):
        """aie_policy_mlp_backward: the gradients of both classes' weights from the gradients with respect to logits and
        values (ppo_loss's grad_logits and grad_values), THREE launches on the current stream.  x_* and weights_* as for
        policy_mlp_forward (the same validation); g_logits_* [rows, M] and g_values_* [rows]: contiguous float32 device
        tensors, g_values exactly for a class with wv.  Returns (grads_a, grads_p): a dict w1, b1, w2, b2, w3, b3 (and wv,
        bv) of new float32 tensors in the weights' shapes per class, None for a class left out; out=(dict_a, dict_p) fills
        the caller's contiguous float32 tensors instead.  Every entry is overwritten.  The arithmetic contract (segments of
        _cabi.MLP_BWD_SEG rows, float64 sums of the segments, no atomics: two runs give the same bits) is include/aie.h's.
        The workspace grows with the row count; it is cached per backend and replaced when a call needs more (calls of one
        backend share it and must not run at the same time on two streams; a captured call keeps the pointer, so capture
        the largest batch first or keep batch sizes fixed)."""
        torch = _torch()
        f = dict(dtype=torch.float32, device=self.device)
        out = tuple(out) if out is not None else (None, None)
        classes, res, Bs = [], [], set()
        for who, x, w, per, gl, gv, o in (("a", x_a, weights_a, self.n, g_logits_a, g_values_a, out[0]),
                                          ("p", x_p, weights_p, 1, g_logits_p, g_values_p, out[1])):
            if x is None:
                classes.append(None)
                res.append(None)
                continue
            x, x_ld, t, F, H, M = self._mlp_operands("policy_mlp_backward", who, x, w, per)
            rows = int(x.shape[0])
            shapes = dict(w1=(F, H), b1=(H,), w2=(H, H), b2=(H,), w3=(H, M), b3=(M,), wv=(H,), bv=(1,))
            has_v = t["wv"] is not None
            if (gv is not None) != has_v:
                raise ValueError("policy_mlp_backward: g_values_%s goes with wv: both or neither" % who)
            for g, numel, what in ((gl, rows * M, "g_logits"), (gv, rows, "g_values")):
                if (g is None and what == "g_logits") or (g is not None and (
                        g.dtype != torch.float32 or g.device != self.device or not g.is_contiguous() or g.numel() != numel)):
                    raise ValueError("policy_mlp_backward: %s_%s must be a contiguous float32 device tensor of %d elements"
                                     % (what, who, numel))
            names = [k for k in shapes if t[k] is not None]
            if o is not None:
                for k in names:
                    v = o.get(k)
                    if (v is None or v.dtype != torch.float32 or v.device != self.device or not v.is_contiguous()
                            or v.numel() != t[k].numel()):
                        raise ValueError("policy_mlp_backward: out's %s_%s must be a contiguous float32 device tensor of %d elements"
                                         % (k, who, t[k].numel()))
                grads = {k: o[k] for k in names}
            else:
                grads = {k: torch.empty_like(t[k]) for k in names}
            ptr = lambda v: v.data_ptr() if v is not None else None  # noqa: E731
            net = _cabi.AieMlpClass(x=x.data_ptr(), x_ld=x_ld, w1=ptr(t["w1"]), b1=ptr(t["b1"]), w2=ptr(t["w2"]), b2=ptr(t["b2"]),
                                    w3=ptr(t["w3"]), b3=ptr(t["b3"]), wv=ptr(t["wv"]), bv=ptr(t["bv"]), logits=None, values=None,
                                    F=F, H=H, M=M)
            classes.append(_cabi.AieMlpGradClass(net=net, g_logits=ptr(gl), g_values=ptr(gv),
                                                 **{"g" + k: ptr(grads.get(k)) for k in shapes}))
            res.append(grads)
            Bs.add(rows // per)
        if not Bs:
            raise ValueError("policy_mlp_backward: no actor class")
        if len(Bs) != 1:
            raise ValueError("policy_mlp_backward: the classes disagree on the batch size (%s)" % sorted(Bs))
        B = C.c_int64(Bs.pop())
        ref = lambda c: C.byref(c) if c is not None else None  # noqa: E731
        need = int(self.lib.aie_policy_mlp_backward_workspace_bytes(self.handle, B, ref(classes[0]), ref(classes[1])))
        ws = getattr(self, "_mlp_bwd_ws", None)
        if need > 0 and (ws is None or ws.numel() * 4 < need):
            ws = self._mlp_bwd_ws = torch.empty((need + 3) // 4, **f)
        # (a refusal of the plan makes `need` its negative code: the call below then refuses too, and names itself)
        self._check(self.lib.aie_policy_mlp_backward(self.handle, B, ref(classes[0]), ref(classes[1]),
                                                     C.c_void_p(ws.data_ptr()) if ws is not None else None,
                                                     C.c_int64(ws.numel() * 4 if ws is not None else 0), self._stream()))
        return res[0], res[1]

    def _action_buffers(self, slot):
        torch = _torch()
        if self._rand_a is None:
            wa = 1 if not self.cfg.multi_action_mode_agents else max(1, self._n_sub_a())
            wp = self._act_p_width()
            self._rand_a = [torch.zeros((self.E, self.n, wa), dtype=torch.int32, device=self.device) for _ in range(2)]
            self._rand_p = [torch.zeros((self.E, wp), dtype=torch.int32, device=self.device) for _ in range(2)]
        return self._rand_a[slot], self._rand_p[slot]

    def sample_random_actions(self, seed, env_offset=0, slot=0):
        """Fills (and returns) caller-owned action buffers with the benchmark's uniform random
        policy.  `slot` selects one of two buffer pairs so that the actions of step t+1 can be
        sampled (on another stream) while step t still reads its own."""
        a, p = self._action_buffers(slot)
        self._check(self.lib.aie_sample_random_actions(
            self.handle, C.c_uint64(seed), C.c_int64(env_offset),
            C.c_void_p(a.data_ptr()), C.c_void_p(p.data_ptr()), self._stream()))
        return a, p

    def _n_sub_a(self):
        comps = list(self.cfg.components)[: self.cfg.n_components]
        return sum({_cabi.COMP_BUILD: 1, _cabi.COMP_CDA: 4, _cabi.COMP_GATHER: 1,
                    _cabi.COMP_SIMPLE_LABOR: 1}.get(c, 0) for c in comps) + int(self.cfg.host_a_n)

    def _act_p_width(self):
        return self._act_p_width_for(self.cfg)

    @staticmethod
    def _act_p_width_for(cfg):
        has_planner_actions = (
            _cabi.COMP_TAX in list(cfg.components)[: cfg.n_components]
            and cfg.tax_model == 0 and not cfg.tax_disable)
        if cfg.multi_action_mode_planner:  # one column per row: the tax brackets and the host components' subspaces
            return max(1, (cfg.tax_n_brackets if has_planner_actions else 0) + int(cfg.host_p_n))
        return 1

    def upload(self, name, array):
        dtype, shape, _, _ = self.descs[name]
        arr = np.ascontiguousarray(np.broadcast_to(np.asarray(array), shape), np.dtype(_cabi.DTYPES[dtype]))
        self._check(self.lib.aie_upload(self.handle, name.encode(), arr.ctypes.data, arr.nbytes))

    def download(self, name):
        dtype, shape, _, _ = self.descs[name]
        arr = np.empty(shape, np.dtype(_cabi.DTYPES[dtype]))
        self._check(self.lib.aie_download(self.handle, name.encode(), arr.ctypes.data, arr.nbytes))
        return arr

    def invalidate_observations(self, e=None):
        """Call after editing state tensors (or overwriting observation tensors) from outside the kernels: the next
        step rewrites the map observations, the action masks and the flat vectors of replica(s) `e` in full instead of
        updating them in place (`obs_valid`).  `upload` of a record field does it for every replica."""
        if "obs_valid" in self.tensors:
            if e is None:
                self.tensors["obs_valid"].zero_()
            else:
                self.tensors["obs_valid"][e] = 0

    def load_state(self, state, e=None):
        """Injects a host state ({field: array without env dim}) into replica e (or all)."""
        torch = _torch()
        self.invalidate_observations(e)
        for k, v in state.items():
            if k in ("stone_src", "wood_src", "water"):
                continue
            if k not in self.tensors:
                continue
            t = self.tensors[k]
            arr = np.asarray(v)
            if k == "mt":
                arr = arr.astype(np.uint32).view(np.int32)
            src = torch.as_tensor(arr, device=self.device).to(t.dtype)
            if e is None:
                t[...] = src
            else:
                t[e] = src
        if "stone_src" in state:
            fl = (np.asarray(state["water"], np.uint8) + 2 * np.asarray(state["stone_src"], np.uint8)
                  + 4 * np.asarray(state["wood_src"], np.uint8)).astype(np.uint8)
            src = torch.as_tensor(fl, device=self.device)
            if self.cfg.shared_layout and self.cfg.layout_gen == _cabi.LAYOUT_FIXED and self.cfg.rng_mode == _cabi.RNG_FAST:
                # one source layout for the whole batch (the regeneration's source list is derived from it once,
                # aie_set_layout): a state that carries another layout cannot be injected into some replicas only
                if not bool((self.tensors["cell_flags"][0 if e is None else e] == src).all()):
                    raise ValueError("load_state: the state's source / water planes differ from the environment's shared "
                                     "layout (shared_layout=1): create the environment with that layout")
            if e is None:
                self.tensors["cell_flags"][...] = src
            else:
                self.tensors["cell_flags"][e] = src
            if "regen_src_list" in self.tensors:
                # the regeneration's source doubles (record fields the reset kernel derives from the flags,
                # csrc/aie_layout.h: o_src_list): Wood cells ascending, then Stone cells
                hw = int(np.asarray(state["wood_src"]).size)
                d = np.concatenate([np.flatnonzero(np.asarray(state["wood_src"]).reshape(-1)),
                                    hw + np.flatnonzero(np.asarray(state["stone_src"]).reshape(-1))])
                cap = int(self.tensors["regen_src_list"].shape[-1])
                lst = np.zeros(cap, np.int16)
                lst[: min(cap, d.size)] = d[:cap].astype(np.uint16).view(np.int16)
                lst_t = torch.as_tensor(lst, device=self.device)
                if e is None:
                    self.tensors["regen_src_list"][...] = lst_t
                    self.tensors["regen_src_n"][...] = int(d.size)
                else:
                    self.tensors["regen_src_list"][e] = lst_t
                    self.tensors["regen_src_n"][e] = int(d.size)
            if "regen_source_count" in self.tensors:
                # bookkeeping the reset kernel derives from the layout (source blocks per regeneration window,
                # csrc/aie_layout.h: regen_conv): a layout injected here needs the same counts
                cnt = self._source_window_counts(np.asarray(state["stone_src"]), np.asarray(state["wood_src"]))
                src = torch.as_tensor(cnt, device=self.device)
                if e is None:
                    self.tensors["regen_source_count"][...] = src
                else:
                    self.tensors["regen_source_count"][e] = src

    def _source_window_counts(self, stone_src, wood_src):
        out = []
        for plane, hw in ((stone_src, int(self.cfg.regen_halfwidth[0])), (wood_src, int(self.cfg.regen_halfwidth[1]))):
            p = np.pad((np.asarray(plane) > 0).astype(np.int32), hw)
            H, W = np.asarray(plane).shape
            acc = np.zeros((H, W), np.int32)
            for dr in range(2 * hw + 1):
                for dc in range(2 * hw + 1):
                    acc += p[dr: dr + H, dc: dc + W]
            out.append(acc)
        return np.stack(out).astype(np.uint8)

    def close(self):
        """Releases the environment.  A library-owned arena (1 GiB and up) is freed when the LAST tensor view of it is
        gone -- action buffers and tensors the caller still holds keep it alive; `free_now()` does not wait for them."""
        if getattr(self, "handle", None):
            if getattr(self, "_arena_owner", None) is not None:
                # the library owns the arena: the handle is destroyed when the last view of the arena is gone
                self._arena_owner = None
                self.arena = None
                self.tensors = {}
                self._rand_a = self._rand_p = None
            else:
                self.lib.aie_destroy(self.handle)
            self.handle = None

    def free_now(self):
        """close() + the memory back NOW (large environments created back to back: a stale view of a library-owned
        7 GB arena would otherwise keep it until the garbage collector finds it).  Views the caller still holds dangle
        afterwards -- use only when none are."""
        import gc

        owner = getattr(self, "_arena_owner", None)
        self.close()
        if owner is not None:
            try:
                _torch().cuda.synchronize(self.device)
            except Exception:
                pass
            h, owner.handle = owner.handle, None  # (the owner's __del__ then has nothing left to destroy)
            if h:
                self.lib.aie_destroy(h)
        gc.collect()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
