"""The trainer operators of the device backend (env.DeviceBackend inherits TrainerOps): policy evaluation and its backward,
trajectory storage, GAE, the PPO loss, the policy MLP, the optimizer step.  A method checks its operands, hands plain pointers to one C ABI call
(the library plans and launches: csrc/aie_trainer_plan.h) and returns torch tensors.  Network outputs and the evaluate calls'
operands are CONVERTED (`.to(...).contiguous()`); stored operands, `out=` tensors and weights are REFUSED unless right."""
import ctypes as C
import math

import numpy as np

from . import _cabi


def ptr(t):  # a tensor's device address for the C ABI (None: NULL)
    return t.data_ptr() if t is not None else None


def ref(c):  # a ctypes structure by reference (None: NULL)
    return C.byref(c) if c is not None else None


def operand(fn, what, t, dtype, device, numel=None, per=None):
    """The ONE operand check: `t` is a contiguous `dtype` tensor on `device` of `numel` elements (or, with `per`, of a positive
    multiple of `per`), else ValueError naming the function and the operand.  Returns t.  device None: an operand this module
    converted itself (`.to(...).contiguous()`), right by construction in all but its element count."""
    right = device is None or (getattr(t, "dtype", None) == dtype and t.device == device and t.is_contiguous())
    n = t.numel() if right else -1
    if (n != numel) if per is None else (n <= 0 or n % per != 0):
        raise ValueError("%s: %s must be a contiguous %s device tensor of %s elements"
                         % (fn, what, dtype, numel if per is None else "a positive multiple of %d" % per))
    return t


class TrainerOps:
    """Mixin of DeviceBackend: uses its lib, handle, device, E, n, tensors, _check, _stream and _action_buffers."""

    def _per_batch_element(self):
        """Elements per batch element: (agents' logits, planner's logits, agents' actions, planner's actions)."""
        aa, ap = self._action_buffers(0)
        return (self.tensors["obs_a_action_mask"].numel() // self.E, self.tensors["obs_p_action_mask"].numel() // self.E,
                aa.numel() // self.E, ap.numel() // self.E)

    def _policy_eval_operands(self, logits_a, logits_p, masks_a, masks_p, actions_a, actions_p):
        """Contiguous device operands of aie_policy_evaluate / _backward and the batch size B they agree on."""
        import torch
        per_a, per_p, act_a, act_p = self._per_batch_element()
        ops, Bs = {}, set()
        for k, t, dtype, per in (("la", logits_a, torch.float32, per_a), ("lp", logits_p, torch.float32, per_p),
                                 ("ma", masks_a, torch.float32, per_a), ("mp", masks_p, torch.float32, per_p),
                                 ("aa", actions_a, torch.int32, act_a), ("ap", actions_p, torch.int32, act_p)):
            if t is not None:
                if not isinstance(t, torch.Tensor):
                    t = torch.as_tensor(np.asarray(t))
                t = operand("policy evaluation", "operand " + k, t.to(device=self.device, dtype=dtype).contiguous(), dtype, None, per=per)
                Bs.add(t.numel() // per)
            ops[k] = t
        if len(Bs) != 1:
            raise ValueError("policy evaluation: the operands disagree on the batch size (%s)" % sorted(Bs))
        return ops, Bs.pop(), (act_a, act_p)

    def policy_evaluate(self, logits_a, logits_p, masks_a, masks_p, actions_a, actions_p, entropy=True):
        """aie_policy_evaluate: (logp_a, logp_p, entropy_a, entropy_p) of stored actions under stored masks for the given
        logits, B batch elements (any B: the operands' leading extent(s); with masks None -- the arena's current masks
        -- B = E).  Layouts as sample_policy_actions / action_masks; either actor class may be None (its outputs are
        None).  One launch on the current stream."""
        import torch
        ops, B, _ = self._policy_eval_operands(logits_a, logits_p, masks_a, masks_p, actions_a, actions_p)
        f = dict(dtype=torch.float32, device=self.device)
        sa, sp = ((B,) + tuple(t.shape[1:]) for t in self._action_buffers(0))
        out = [torch.empty(sa, **f) if ops["la"] is not None and ops["aa"] is not None else None,
               torch.empty(sp, **f) if ops["lp"] is not None and ops["ap"] is not None else None,
               torch.empty(sa, **f) if ops["la"] is not None and entropy else None,
               torch.empty(sp, **f) if ops["lp"] is not None and entropy else None]
        self._check(self.lib.aie_policy_evaluate(
            self.handle, B, ptr(ops["la"]), ptr(ops["lp"]), ptr(ops["ma"]), ptr(ops["mp"]), ptr(ops["aa"]), ptr(ops["ap"]),
            ptr(out[0]), ptr(out[1]), ptr(out[2]), ptr(out[3]), self._stream()))
        return tuple(out)

    def policy_evaluate_backward(self, logits_a, logits_p, masks_a, masks_p, actions_a, actions_p,
                                 g_logp_a=None, g_logp_p=None, g_entropy_a=None, g_entropy_p=None):
        """aie_policy_evaluate_backward: (grad_logits_a, grad_logits_p), the logits' shapes, of
        sum(g_logp * logp + g_entropy * entropy); a None gradient counts as zeros.  One launch on the current stream."""
        import torch
        ops, B, (act_a, act_p) = self._policy_eval_operands(logits_a, logits_p, masks_a, masks_p, actions_a, actions_p)
        gs = []
        for g, per, what in ((g_logp_a, act_a, "g_logp_a"), (g_logp_p, act_p, "g_logp_p"), (g_entropy_a, act_a, "g_entropy_a"),
                             (g_entropy_p, act_p, "g_entropy_p")):
            if g is not None:
                g = operand("policy_evaluate_backward", what, g.to(self.device, torch.float32).contiguous(), torch.float32, None, B * per)
            gs.append(g)
        grad_a = torch.empty_like(ops["la"]) if ops["la"] is not None else None
        grad_p = torch.empty_like(ops["lp"]) if ops["lp"] is not None else None
        self._check(self.lib.aie_policy_evaluate_backward(
            self.handle, B, ptr(ops["la"]), ptr(ops["lp"]), ptr(ops["ma"]), ptr(ops["mp"]), ptr(ops["aa"]), ptr(ops["ap"]),
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
        import torch
        segs = [s[0] if isinstance(s, tuple) else s for s in segments]
        operand("trajectory_store", "slot_counters", slot_counters, torch.int32, self.device, self.E)
        arr = (_cabi.AieTrajSegment * max(1, len(segs)))(*segs)
        self._check(self.lib.aie_trajectory_store(self.handle, arr, len(segs), int(n_slots), ptr(slot_counters), self._stream()))

    def gae(self, T, log, values_a, values_p, gamma, lam, first_slot=0, advantages=True, returns=True, out=None):
        """aie_gae: (adv_a, adv_p, ret_a, ret_p) of T steps from a reward log (float32 [n_slots, E, n + 2], time t in slot
        (first_slot + t) % n_slots) and the values (float32 [T + 1, E, n] / [T + 1, E], row T the bootstrap; either may be
        None).  One launch on the current stream.  out=(adv_a, adv_p, ret_a, ret_p) to fill the caller's own."""
        import torch
        T, f = int(T), dict(dtype=torch.float32, device=self.device)
        operand("gae", "the log", log, torch.float32, self.device, per=self.E * (self.n + 2))
        if log.dim() != 3 or tuple(log.shape[1:]) != (self.E, self.n + 2):
            raise ValueError("gae: the log is a contiguous float32 device tensor [n_slots, %d, %d]" % (self.E, self.n + 2))
        for v, per, what in ((values_a, self.E * self.n, "values_a"), (values_p, self.E, "values_p")):
            if v is not None:
                operand("gae", what, v, torch.float32, self.device, (T + 1) * per)
        if out is None:
            sa, sp = (T, self.E, self.n), (T, self.E)
            out = [torch.empty(sa, **f) if values_a is not None and advantages else None,
                   torch.empty(sp, **f) if values_p is not None and advantages else None,
                   torch.empty(sa, **f) if values_a is not None and returns else None,
                   torch.empty(sp, **f) if values_p is not None and returns else None]
        else:
            for o, per, what in zip(out, (self.E * self.n, self.E) * 2, ("adv_a", "adv_p", "ret_a", "ret_p")):
                if o is not None:
                    operand("gae", what, o, torch.float32, self.device, T * per)
        self._check(self.lib.aie_gae(self.handle, T, ptr(log), int(log.shape[0]), int(first_slot), ptr(values_a), ptr(values_p),
                                     gamma, lam, ptr(out[0]), ptr(out[1]), ptr(out[2]), ptr(out[3]), self._stream()))
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
        import torch
        per_a, per_p, act_a, act_p = self._per_batch_element()
        f = dict(dtype=torch.float32, device=self.device)  # (the network's outputs: made contiguous float32 here if they are not)
        la = operand("ppo_loss", "logits_a", logits_a.detach().to(**f).contiguous(), torch.float32, None, per=per_a) \
            if logits_a is not None else None
        lp = operand("ppo_loss", "logits_p", logits_p.detach().to(**f).contiguous(), torch.float32, None, per=per_p) \
            if logits_p is not None else None
        if la is None and lp is None:
            raise ValueError("ppo_loss: no actor class")
        va = operand("ppo_loss", "values_a", values_a.detach().to(**f).contiguous(), torch.float32, None, per=self.n) \
            if la is not None and values_a is not None else None
        vp = operand("ppo_loss", "values_p", values_p.detach().to(**f).contiguous(), torch.float32, None, per=1) \
            if lp is not None and values_p is not None else None
        Bs = {t.numel() // per for t, per in ((la, per_a), (lp, per_p), (va, self.n), (vp, 1)) if t is not None}
        if len(Bs) != 1:
            raise ValueError("ppo_loss: logits and values disagree on the batch size (%s)" % sorted(Bs))
        B = Bs.pop()
        if index is not None:
            operand("ppo_loss", "index", index, torch.int32, self.device, B)
        mom = adv_moments if adv_moments is not None else (None, None)
        coef_a = dict(clip=clip, vf_clip=vf_clip, vf_coef=vf_coef, ent_coef=ent_coef)
        coef_p = dict(coef_a, **coeffs_p) if coeffs_p else coef_a
        classes, outs, Rs = [], [], set()
        for who, lg, val, per, act, actors, co, mo in (("a", la, va, per_a, act_a, self.n, coef_a, mom[0]),
                                                       ("p", lp, vp, per_p, act_p, 1, coef_p, mom[1])):
            if lg is None:
                classes.append(None)
                outs.append(None)
                continue
            ops = {}  # the stored operands: used where they lie (one the batch does not have is refused like a wrong one)
            for name, dtype, n_per in (("masks", torch.float32, per), ("actions", torch.int32, act), ("logp_old", torch.float32, act),
                                       ("adv", torch.float32, actors), ("values_old", torch.float32, actors),
                                       ("returns", torch.float32, actors))[:6 if val is not None else 4]:
                key = name + "_" + who
                ops[name] = operand("ppo_loss", key, batch.get(key), dtype, self.device, per=n_per)
                Rs.add(ops[name].numel() // n_per)
            if mo is not None:
                operand("ppo_loss", "adv_moments {mean, rstd}", mo, torch.float32, self.device, 2)
            if out is not None:
                stats, grad, grad_v = out[who == "p"]
                if (grad_v is None) != (val is None):
                    raise ValueError("ppo_loss: out's grad_values_%s goes with values: both or neither" % who)
                for t, numel, what in ((stats, _cabi.PPO_N_STATS, "out's stats_"), (grad, lg.numel(), "out's grad_logits_"),
                                       (grad_v, val.numel() if val is not None else 0, "out's grad_values_"))[:3 if val is not None else 2]:
                    operand("ppo_loss", what + who, t, torch.float32, self.device, numel)
            else:
                stats, grad = torch.empty(_cabi.PPO_N_STATS, **f), torch.empty_like(lg)
                grad_v = torch.empty_like(val) if val is not None else None
            classes.append(_cabi.AiePpoClass(
                logits=ptr(lg), values=ptr(val), masks=ptr(ops["masks"]), actions=ptr(ops["actions"]), logp_old=ptr(ops["logp_old"]),
                adv=ptr(ops["adv"]), values_old=ptr(ops.get("values_old")), returns=ptr(ops.get("returns")), adv_moments=ptr(mo),
                grad_logits=ptr(grad), grad_values=ptr(grad_v), stats=ptr(stats), clip=co["clip"], vf_clip=co["vf_clip"],
                vf_coef=co["vf_coef"], ent_coef=co["ent_coef"]))
            outs.append((stats, grad, grad_v))
        if len(Rs) != 1 or (index is None and Rs != {B}):
            raise ValueError("ppo_loss: the stored operands have %s rows; all must agree, and without an index equal B = %d"
                             % (sorted(Rs), B))
        # the workspace: the largest any B needs (1 MiB), allocated once per backend and never replaced -- a captured call keeps
        # its pointer.  Calls of one backend share it: they must not overlap (two streams: two workspaces through the C ABI)
        ws = getattr(self, "_ppo_ws", None)
        if ws is None:
            ws = self._ppo_ws = torch.empty(_cabi.PPO_MAX_WAVES * 16, dtype=torch.float64, device=self.device)
        self._check(self.lib.aie_ppo_loss(self.handle, B, ref(classes[0]), ref(classes[1]), ptr(index), ptr(ws), ws.numel() * 8,
                                          self._stream()))
        return outs[0], outs[1]

    def _mlp_operands(self, fn, who, x, w, per):
        """One class of policy_mlp_forward / policy_mlp_backward: the checks they share -> (the finished _cabi.AieMlpClass
        with logits and values NULL: the forward fills them in; the dict of its weight tensors w1 .. bv; rows; M)."""
        import torch
        get = w.get if hasattr(w, "get") else lambda k, w=w: getattr(w, k, None)  # noqa: E731
        if x.dim() == 3:  # [B, n, F] with one row stride throughout: a view, never a copy
            if x.shape[0] > 1 and x.stride(0) != x.shape[1] * x.stride(1):
                raise ValueError("%s: x_%s [B, n, F] needs one row stride throughout (strides %s)" % (fn, who, tuple(x.stride())))
            x = x.as_strided((x.shape[0] * x.shape[1], x.shape[2]), (x.stride(1), x.stride(2)), x.storage_offset())
        if x.dim() != 2 or x.dtype != torch.float32 or x.device != self.device or (x.shape[1] > 1 and x.stride(1) != 1) \
                or x.shape[0] == 0 or x.shape[0] % per:
            raise ValueError("%s: x_%s is a float32 device tensor [B x %d, F] with contiguous rows" % (fn, who, per))
        rows, F = int(x.shape[0]), int(x.shape[1])
        t = {k: get(k) for k in ("w1", "b1", "w2", "b2", "w3", "b3", "wv", "bv")}
        H = int(t["w1"].shape[-1]) if t["w1"] is not None and t["w1"].dim() == 2 else 0
        M = int(t["w3"].shape[-1]) if t["w3"] is not None and t["w3"].dim() == 2 else 0
        for k, shape in (("w1", (F, H)), ("b1", (H,)), ("w2", (H, H)), ("b2", (H,)), ("w3", (H, M)), ("b3", (M,)),
                         ("wv", (H,)), ("bv", (1,))):
            v = t[k]
            if v is None and k in ("wv", "bv"):
                continue
            operand(fn, "weights_" + who + "." + k, v, torch.float32, self.device, math.prod(shape))
            if v.dim() == 2 and k != "wv" and tuple(v.shape) != shape:
                raise ValueError("%s: weights_%s[%r] must have the shape %s" % (fn, who, k, shape))
        if (t["wv"] is None) != (t["bv"] is None):
            raise ValueError("%s: weights_%s needs wv and bv together" % (fn, who))
        net = _cabi.AieMlpClass(x=x.data_ptr(), x_ld=int(x.stride(0)) if rows > 1 else F, w1=ptr(t["w1"]), b1=ptr(t["b1"]),
                                w2=ptr(t["w2"]), b2=ptr(t["b2"]), w3=ptr(t["w3"]), b3=ptr(t["b3"]), wv=ptr(t["wv"]), bv=ptr(t["bv"]),
                                logits=None, values=None, F=F, H=H, M=M)
        return net, t, rows, M

    @staticmethod
    def _one_batch_size(fn, Bs):
        if not Bs:
            raise ValueError("%s: no actor class" % fn)
        if len(Bs) != 1:
            raise ValueError("%s: the classes disagree on the batch size (%s)" % (fn, sorted(Bs)))
        return Bs.pop()

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
        import torch
        fn = "policy_mlp_forward"
        f = dict(dtype=torch.float32, device=self.device)
        out = tuple(out) if out is not None else (None,) * 4
        classes, res, Bs = [], [], set()
        for who, x, w, per, o_l, o_v in (("a", x_a, weights_a, self.n, out[0], out[2]), ("p", x_p, weights_p, 1, out[1], out[3])):
            if x is None:
                classes.append(None)
                res.append((None, None))
                continue
            net, t, rows, M = self._mlp_operands(fn, who, x, w, per)
            for o, numel, what in ((o_l, rows * M, "logits"), (o_v, rows, "value")):
                if o is not None:
                    operand(fn, "out's " + what + "_" + who, o, torch.float32, self.device, numel)
            logits = o_l if o_l is not None else torch.empty((rows, M), **f)
            value = (o_v if o_v is not None else torch.empty((rows,), **f)) if t["wv"] is not None else None
            net.logits, net.values = ptr(logits), ptr(value)
            classes.append(net)
            res.append((logits, value))
            Bs.add(rows // per)
        B = self._one_batch_size(fn, Bs)
        self._check(self.lib.aie_policy_mlp_forward(self.handle, B, ref(classes[0]), ref(classes[1]), self._stream()))
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
        import torch
        fn = "policy_mlp_backward"
        out = tuple(out) if out is not None else (None, None)
        classes, res, Bs = [], [], set()
        for who, x, w, per, gl, gv, o in (("a", x_a, weights_a, self.n, g_logits_a, g_values_a, out[0]),
                                          ("p", x_p, weights_p, 1, g_logits_p, g_values_p, out[1])):
            if x is None:
                classes.append(None)
                res.append(None)
                continue
            net, t, rows, M = self._mlp_operands(fn, who, x, w, per)
            if (gv is not None) != (t["wv"] is not None):
                raise ValueError("policy_mlp_backward: g_values_%s goes with wv: both or neither" % who)
            operand(fn, "g_logits_" + who, gl, torch.float32, self.device, rows * M)
            if gv is not None:
                operand(fn, "g_values_" + who, gv, torch.float32, self.device, rows)
            names = [k for k in t if t[k] is not None]
            if o is not None:
                grads = {k: operand(fn, "out's " + k + "_" + who, o.get(k), torch.float32, self.device, t[k].numel()) for k in names}
            else:
                grads = {k: torch.empty_like(t[k]) for k in names}
            classes.append(_cabi.AieMlpGradClass(net=net, g_logits=ptr(gl), g_values=ptr(gv),
                                                 **{"g" + k: ptr(grads.get(k)) for k in t}))
            res.append(grads)
            Bs.add(rows // per)
        B = self._one_batch_size(fn, Bs)
        need = int(self.lib.aie_policy_mlp_backward_workspace_bytes(self.handle, B, ref(classes[0]), ref(classes[1])))
        ws = getattr(self, "_mlp_bwd_ws", None)
        if need > 0 and (ws is None or ws.numel() * 4 < need):
            ws = self._mlp_bwd_ws = torch.empty((need + 3) // 4, dtype=torch.float32, device=self.device)
        # (a refusal of the plan makes `need` its negative code: the call below then refuses too, and names itself)
        self._check(self.lib.aie_policy_mlp_backward(self.handle, B, ref(classes[0]), ref(classes[1]), ptr(ws),
                                                     ws.numel() * 4 if ws is not None else 0, self._stream()))
        # what policy_mlp_input_grad, directly behind this call, reads: the classes (plain pointers: no tensor is kept alive
        # by them; that call reads only w1 and the workspace), B and the workspace
        self._mlp_bwd_last = (classes, B, ws)
        return res[0], res[1]

    def policy_mlp_input_grad(self, ncols_a=None, ncols_p=None, out=None):
        """aie_policy_mlp_input_grad: the gradient with respect to the first ncols columns of x, for a network in front of the
        MLP -- ONE launch on the current stream, valid only DIRECTLY BEHIND policy_mlp_backward on the same stream: it reads
        dz1 from that call's workspace and uses that call's classes (their pointers, not their tensors: the weights of that
        call must still be alive, nothing else is read).  ncols_* None: the class is left out.  Returns
        (g_x_a [rows_a, ncols_a], g_x_p [B, ncols_p]), None for a class left out; out=(g_x_a, g_x_p) fills the caller's
        float32 device tensors [rows, >= ncols] with contiguous rows (any row stride) instead."""
        import torch
        fn = "policy_mlp_input_grad"
        last = getattr(self, "_mlp_bwd_last", None)
        if last is None:
            raise ValueError("%s: call policy_mlp_backward first" % fn)
        classes, B, ws = last
        out = tuple(out) if out is not None else (None, None)
        args, res = [], []
        for who, cls, per, ncols, o in (("a", classes[0], self.n, ncols_a, out[0]), ("p", classes[1], 1, ncols_p, out[1])):
            if ncols is None:
                args += [None, 0, 0]
                res.append(None)
                continue
            if cls is None:
                raise ValueError("%s: ncols_%s without that class in the backward" % (fn, who))
            rows = B * per
            if o is None:
                o = torch.empty((rows, int(ncols)), dtype=torch.float32, device=self.device)
            elif not (o.dim() == 2 and o.dtype == torch.float32 and o.device == self.device and o.shape[0] == rows
                      and o.shape[1] >= ncols and (o.shape[1] == 1 or o.stride(1) == 1)):
                raise ValueError("%s: out's g_x_%s is a float32 device tensor [%d, >= %d] with contiguous rows" % (fn, who, rows, ncols))
            args += [ptr(o), int(o.stride(0)) if rows > 1 else int(o.shape[1]), int(ncols)]
            res.append(o)
        self._check(self.lib.aie_policy_mlp_input_grad(self.handle, B, ref(classes[0]), ref(classes[1]), ptr(ws),
                                                       ws.numel() * 4 if ws is not None else 0, *args, self._stream()))
        return res[0], res[1]

    def _conv_rows(self, fn, what, t, dtype, inner):
        """A crop operand [rows, *inner] or [B, n, *inner] with each row's block contiguous and one row stride throughout: a
        view, never a copy -> (the tensor, rows, the row stride in elements)."""
        k = len(inner)
        ok = getattr(t, "dtype", None) == dtype and t.device == self.device and t.dim() in (k + 1, k + 2) \
            and tuple(t.shape[-k:]) == tuple(inner) and t[(0,) * (t.dim() - k)].is_contiguous() and t.numel() > 0
        if ok and t.dim() == k + 2 and t.shape[0] > 1 and t.shape[1] > 1 and t.stride(0) != t.shape[1] * t.stride(1):
            ok = False
        if not ok:
            raise ValueError("%s: %s is a %s device tensor [rows, %s] (or [B, n, ...]) whose rows are contiguous blocks one stride apart"
                             % (fn, what, dtype, ", ".join(map(str, inner))))
        rows = math.prod(t.shape[:-k])
        lead = t.dim() - k
        stride = t.stride(lead - 1) if t.shape[lead - 1] > 1 else (t.stride(0) if lead == 2 and t.shape[0] > 1 else math.prod(inner))
        return t, rows, int(stride)

    def _conv_operands(self, fn, map_, idx, w):
        """What policy_conv_forward / policy_conv_backward share -> (a _cabi.AieConvClass without flat and x_out, the dict
        of the five weight tensors, rows, NF)."""
        import torch
        get = w.get if hasattr(w, "get") else lambda k, w=w: getattr(w, k, None)  # noqa: E731
        t = {k: get(k) for k in ("emb", "w1", "b1", "w2", "b2")}
        if getattr(map_, "dim", lambda: 0)() < 4 or t["emb"] is None or t["emb"].dim() != 2:
            raise ValueError("%s: map [rows, C_map, h, w] and conv_weights with emb [V, D], w1, b1, w2, b2" % fn)
        C_map, h, w_ = (int(v) for v in map_.shape[-3:])
        V, D = (int(v) for v in t["emb"].shape)
        _, rows, map_ld = self._conv_rows(fn, "map", map_, torch.float32, (C_map, h, w_))
        _, rows_i, idx_ld = self._conv_rows(fn, "idx", idx, torch.int16, (2, h, w_))
        if rows_i != rows:
            raise ValueError("%s: map has %d rows, idx %d" % (fn, rows, rows_i))
        C = C_map + 2 * D
        for k, shape in (("emb", (V, D)), ("w1", (9 * C, _cabi.CONV_F1)), ("b1", (_cabi.CONV_F1,)),
                         ("w2", (9 * _cabi.CONV_F1, _cabi.CONV_F2)), ("b2", (_cabi.CONV_F2,))):
            operand(fn, "conv_weights." + k, t[k], torch.float32, self.device, math.prod(shape))
            if tuple(t[k].shape) != shape:
                raise ValueError("%s: conv_weights[%r] must have the shape %s" % (fn, k, shape))
        oh1, ow1 = (h - 3) // 2 + 1, (w_ - 3) // 2 + 1
        NF = max(0, ((oh1 - 3) // 2 + 1) * ((ow1 - 3) // 2 + 1)) * _cabi.CONV_F2
        net = _cabi.AieConvClass(map=map_.data_ptr(), map_ld=map_ld, idx=idx.data_ptr(), idx_ld=idx_ld, emb=ptr(t["emb"]),
                                 w1=ptr(t["w1"]), b1=ptr(t["b1"]), w2=ptr(t["w2"]), b2=ptr(t["b2"]), flat=None, flat_ld=0,
                                 x_out=None, x_ld=0, C_map=C_map, D=D, h=h, w=w_, V=V, F_flat=0)
        return net, t, rows, NF

    def policy_conv_forward(self, map, idx, flat, conv_weights, out=None):  # noqa: A002
        """aie_policy_conv_forward: the convolutional encoder of the agents' egocentric crop -- embedding of the two index
        planes, two 3x3 stride-2 convolutions (16, then 32 filters) with ReLU, Keras' flatten -- in ONE launch on the current
        stream.  map: float32 [rows, C_map, h, w] (or [B, n, C_map, h, w]) and idx: int16 [rows, 2, h, w]: device tensors
        used where they lie (the arena's obs_a_world-map / obs_a_world-idx_map, a trajectory's stored copies, any view
        whose rows are contiguous blocks one stride apart); flat: float32 [rows, F_flat] (or [B, n, F_flat]) with contiguous
        rows, or None.  conv_weights: a mapping (or rollout.conv_weights) with float32 device tensors emb [V, D],
        w1 [9 (C_map + 2 D), 16], b1 [16], w2 [144, 32], b2 [32], contiguous, read where they lie at every launch.
        Returns x [rows, NF + F_flat]: the features, then a copy of the flat row -- a legal x_a of policy_mlp_forward;
        out= fills the caller's float32 device tensor [rows, >= NF + F_flat] with contiguous rows instead (columns behind are
        left alone).  Nothing is converted.  The arithmetic contract and the supported shapes are include/aie.h's."""
        import torch
        fn = "policy_conv_forward"
        net, _, rows, NF = self._conv_operands(fn, map, idx, conv_weights)
        F_flat = 0
        if flat is not None:
            if getattr(flat, "dim", lambda: 0)() not in (2, 3):
                raise ValueError("%s: flat is a float32 device tensor [rows, F_flat] (or [B, n, F_flat])" % fn)
            flat, r2, ld = self._conv_rows(fn, "flat", flat, torch.float32, (int(flat.shape[-1]),))
            if r2 != rows:
                raise ValueError("%s: flat must have map's %d rows" % (fn, rows))
            F_flat = int(flat.shape[-1])
            net.flat, net.flat_ld, net.F_flat = flat.data_ptr(), ld, F_flat
        if out is None:
            out = torch.empty((rows, NF + F_flat), dtype=torch.float32, device=self.device)
        elif not (out.dim() == 2 and out.dtype == torch.float32 and out.device == self.device and out.shape[0] == rows
                  and out.shape[1] >= NF + F_flat and out.stride(1) == 1):
            raise ValueError("%s: out is a float32 device tensor [%d, >= %d] with contiguous rows" % (fn, rows, NF + F_flat))
        net.x_out, net.x_ld = out.data_ptr(), int(out.stride(0)) if rows > 1 else int(out.shape[1])
        self._check(self.lib.aie_policy_conv_forward(self.handle, rows, C.byref(net), self._stream()))
        return out

    def policy_conv_backward(self, map, idx, conv_weights, g_feat, out=None):  # noqa: A002
        """aie_policy_conv_backward: the gradients of the encoder's five tensors from g_feat, the gradient with respect to
        its NF features (policy_mlp_input_grad's first NF columns) -- THREE launches on the current stream.  map, idx and
        conv_weights as for policy_conv_forward (the same validation); g_feat: a float32 device tensor [rows, >= NF] with
        contiguous rows (any row stride).  Returns a dict emb, w1, b1, w2, b2 of new float32 tensors in the weights' shapes;
        out= (such a dict) fills the caller's contiguous float32 tensors instead.  Every entry is overwritten.  The
        arithmetic contract (segments of _cabi.MLP_BWD_SEG rows, float64 sums of the segments, no atomics: two runs give the
        same bits) is include/aie.h's.  The workspace grows with the row count; it is cached per backend and replaced when
        a call needs more (policy_mlp_backward's rules: one stream at a time, capture the largest batch first)."""
        import torch
        fn = "policy_conv_backward"
        net, t, rows, NF = self._conv_operands(fn, map, idx, conv_weights)
        if not (getattr(g_feat, "dim", lambda: 0)() == 2 and g_feat.dtype == torch.float32 and g_feat.device == self.device
                and g_feat.shape[0] == rows and g_feat.shape[1] >= NF and g_feat.stride(1) == 1):
            raise ValueError("%s: g_feat is a float32 device tensor [%d, >= %d] with contiguous rows" % (fn, rows, NF))
        if out is not None:
            grads = {k: operand(fn, "out's " + k, out.get(k), torch.float32, self.device, t[k].numel()) for k in t}
        else:
            grads = {k: torch.empty_like(t[k]) for k in t}
        q = _cabi.AieConvGradClass(net=net, g_feat=g_feat.data_ptr(), g_ld=int(g_feat.stride(0)) if rows > 1 else int(g_feat.shape[1]),
                                   **{"g" + k: ptr(grads[k]) for k in t})
        need = int(self.lib.aie_policy_conv_backward_workspace_bytes(self.handle, rows, C.byref(q)))
        ws = getattr(self, "_conv_bwd_ws", None)
        if need > 0 and (ws is None or ws.numel() * 4 < need):
            ws = self._conv_bwd_ws = torch.empty((need + 3) // 4, dtype=torch.float32, device=self.device)
        self._check(self.lib.aie_policy_conv_backward(self.handle, rows, C.byref(q), ptr(ws), ws.numel() * 4 if ws is not None else 0,
                                                      self._stream()))
        return grads

    def adam_group(self, tensors, lr, state, stats, betas=(0.9, 0.999), eps=1e-8, max_norm=0.0):
        """One aie_opt_group for adam_step.  tensors: a sequence of (w, g, m, v), at most _cabi.OPT_MAX_TENSORS, each four
        contiguous float32 device tensors of one element count; lr: a float32 device tensor of one element; state: an
        int64 device tensor of _cabi.OPT_STATE_BYTES // 8 elements, zeroed by the caller before the first step; stats: a
        float32 device tensor of _cabi.OPT_N_STATS elements.  Nothing is converted: a tensor of another dtype, device or
        layout is an error.  Returns (the structure, what it points at): keep the pair alive while a call may use it."""
        import torch
        fn = "adam_step"
        tensors = [tuple(q) for q in tensors]
        if not 1 <= len(tensors) <= _cabi.OPT_MAX_TENSORS or any(len(q) != 4 for q in tensors):
            raise ValueError("%s: a group is 1 .. %d tensors, each (w, g, m, v)" % (fn, _cabi.OPT_MAX_TENSORS))
        arr = (_cabi.AieOptTensor * len(tensors))()
        for i, (w, g, m, v) in enumerate(tensors):
            n = w.numel() if hasattr(w, "numel") else -1
            for what, t in (("w", w), ("g", g), ("m", m), ("v", v)):
                operand(fn, "tensor %d's %s" % (i, what), t, torch.float32, self.device, max(n, 1))
            arr[i] = _cabi.AieOptTensor(ptr(w), ptr(g), ptr(m), ptr(v), n)
        operand(fn, "lr", lr, torch.float32, self.device, 1)
        operand(fn, "state", state, torch.int64, self.device, _cabi.OPT_STATE_BYTES // 8)
        operand(fn, "stats", stats, torch.float32, self.device, _cabi.OPT_N_STATS)
        group = _cabi.AieOptGroup(tensors=arr, n_tensors=len(tensors), beta1=betas[0], beta2=betas[1], eps=eps, max_norm=max_norm,
                                  d_lr=ptr(lr), d_state=ptr(state), d_stats=ptr(stats))
        return group, (arr, tensors, lr, state, stats)

    def adam_workspace_bytes(self, group_a, group_p):
        """aie_adam_workspace_bytes for two adam_group structures (either None)."""
        g = [x[0] if isinstance(x, tuple) else x for x in (group_a, group_p)]
        return int(self.lib.aie_adam_workspace_bytes(self.handle, ref(g[0]), ref(g[1])))

    def adam_step(self, group_a, group_p, workspace):
        """aie_adam_step: one Adam step under a gradient-norm clip, in place, for the agents' and the planner's parameter
        group (what adam_group returns; either None) -- TWO launches on the current stream for both groups together,
        capturable: the step count, the bias-correction products and the learning rate live in device memory, so a replay
        advances them and a schedule is lr.fill_(x).  workspace: a float64 device tensor of at least
        adam_workspace_bytes(...) bytes, the call's own until it has run.  The arithmetic contract (the norm's fixed order,
        every float32 operation rounded on its own, a group with a non-finite norm skipped: two runs give the same bits)
        is include/aie.h's.  The gradients are neither modified nor zeroed."""
        import torch
        g = [x[0] if isinstance(x, tuple) else x for x in (group_a, group_p)]
        if g[0] is None and g[1] is None:
            raise ValueError("adam_step: no parameter group")
        operand("adam_step", "the workspace", workspace, torch.float64, self.device, per=1)
        self._check(self.lib.aie_adam_step(self.handle, ref(g[0]), ref(g[1]), ptr(workspace), workspace.numel() * 8, self._stream()))
