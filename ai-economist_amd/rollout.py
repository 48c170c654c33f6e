"""Trainer-facing rollout loop: policy -> env.step with NOTHING on the host between the steps.

The reference's GPU trainer calls, per step, `sample actions from the policy` then `env_wrapper.step_all_envs()`
(ai_economist/training/training_script.py:88-133 builds that trainer; F/env_wrapper.py:355-377 is the step it drives),
each a handful of kernel launches issued from Python.  At 25 us per environment step the host is the bottleneck long
before the GPU is.  `GraphedStep` captures one iteration -- the caller's policy (any torch code that reads the
observation tensors and writes the action buffers), `aie_step`, and the masked reset of the replicas that finished --
into a hipGraph once and replays it: one host call per environment step, or per `unroll` steps.

Replay-safety is a property of the C ABI, not of this wrapper: aie_step takes nothing by value that changes from step
to step (the random-policy draw index and the reward-log slot are per-replica record fields the kernels advance
themselves, include/aie.h), and never loads code or synchronises.  tests/test_gpu_parity.py:
test_step_is_hipgraph_replayable replays a captured loop against its eager twin and the oracle.

torch is plumbing here (streams, graph capture, the policy network); the environment step is the HIP kernel.
"""


class GraphedStep:
    def __init__(self, env, policy, auto_reset=True, unroll=1, warmup=3, trajectory=None):
        """env: a batched environment (foundation.make_env_instance(..., n_envs=E)), already reset.
        policy(tensors, actions_a, actions_p): reads observation tensors (env.backend.tensors: "obs_a_flat",
        "obs_a_action_mask", "obs_p_flat", ... zero-copy views of the arena) and writes int32 actions IN PLACE into
        actions_a [E, n, width] / actions_p [E, width_p].  It is captured: no host synchronisation, no data-dependent
        Python control flow, fixed shapes.
        auto_reset: replicas restart right behind the step that ends their episode (aie_set_auto_reset).
        unroll: environment steps per replay.
        trajectory: a `Trajectory` of this environment, or None.  With one, an iteration is policy -> trajectory.store(...)
        -> step: the observations and masks the policy saw, its actions and -- where the trajectory keeps them -- the
        policy's `logp_a` / `logp_p` and `value_a` / `value_p` tensors go into the trajectory's next slot, one more launch
        per step, inside the graph.  The warm-up iterations are real steps and real stores: call trajectory.rewind() (and
        reset the environment, if a clean start is wanted) after construction, before the first fragment."""
        import torch

        if env.backend.host_components:  # (its captured aie_step and auto-reset would skip their hooks)
            raise NotImplementedError("GraphedStep: the environment has host components (%s), which run between launches "
                                      "issued from Python: step it with env.step / env.reset"
                                      % ", ".join(env.backend.host_components))
        self.trajectory = trajectory
        if trajectory is not None:  # (checked before anything about the environment changes)
            if trajectory.be is not env.backend:
                raise ValueError("GraphedStep: the trajectory belongs to another environment")
            for flag, names in ((trajectory.has_logp, ("logp_a", "logp_p")), (trajectory.has_values, ("value_a", "value_p"))):
                for name in names:
                    if flag and getattr(policy, name, None) is None:
                        raise ValueError("GraphedStep: the trajectory stores %s but the policy has no tensor attribute of that "
                                         "name (MaskedMLPPolicy: record_logp=True / value_head=True)" % name)
        self.torch = torch
        self.env, self.be = env, env.backend
        self.policy = policy
        self.unroll = int(unroll)
        be = self.be
        if auto_reset:
            be.set_auto_reset(True)
        # The capture records whichever step kernel is current and replays it forever, and auto-reset restarts replicas
        # without passing through aie_reset (where a finished background specialisation is adopted otherwise): wait for
        # the configuration's specialised kernels here, best effort (the generic kernel gives the same results)
        self.specialised = bool(be.specialize(required=False))
        self.actions_a, self.actions_p = be._action_buffers(0)
        self.graph = None
        self._capture(warmup)

    def _iteration(self):
        self.policy(self.be.tensors, self.actions_a, self.actions_p)
        traj = self.trajectory
        if traj is not None:
            pol = self.policy
            traj.store(self.actions_a, self.actions_p,
                       pol.logp_a if traj.has_logp else None, pol.logp_p if traj.has_logp else None,
                       pol.value_a if traj.has_values else None, pol.value_p if traj.has_values else None)
        self.be.step(self.actions_a, self.actions_p)

    def eager(self, iterations=1):
        """The same iteration issued call by call (what the capture recorded): `iterations` x unroll steps."""
        for _ in range(iterations * self.unroll):
            self._iteration()

    def _capture(self, warmup):
        torch = self.torch
        # torch's capture protocol: run the work a few times on a side stream first (lazy initialisations -- cuBLAS/
        # hipBLASLt handles, allocator pools -- must not happen inside the capture); the warm-up iterations ARE
        # environment steps (the caller resets afterwards if it wants a clean start)
        side = torch.cuda.Stream(device=self.be.device)
        side.wait_stream(torch.cuda.current_stream(self.be.device))
        with torch.cuda.stream(side):
            for _ in range(max(0, warmup)):
                self._iteration()
        torch.cuda.current_stream(self.be.device).wait_stream(side)
        torch.cuda.synchronize(self.be.device)
        self.warmup_steps = max(0, warmup)
        self.graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(self.graph):
            for _ in range(self.unroll):
                self._iteration()

    def replay(self, n=1):
        """n replays = n * unroll environment steps; asynchronous like every other call."""
        for _ in range(n):
            self.graph.replay()


class Trajectory:
    """A rollout fragment of T steps in device memory, filled from INSIDE a captured iteration: one aie_trajectory_store
    launch per step copies what the policy saw and did into the next slot of ring buffers whose slot index is a
    per-replica counter on the device (a captured `buf[t].copy_(x)` would freeze t), and the step kernel writes (rewards,
    planner reward, done) of the same step into the same slot of a reward log of exactly T slots, so both rings wrap
    together.  aie_gae then turns the log and the stored values into advantages and returns in one launch.

        obs[name]   [T, E, ...]     any arena tensor (`observations`), the tensor's dtype, as the policy saw it at step t
        masks_a     [T, E, n, MA]   masks_p [T, E, MP]   the action masks in the LOGITS' layout (== Backend.action_masks();
                                    COVID's collated rows are transposed on the way)
        actions_a / actions_p       int32, the action buffers' shapes behind [T]
        logp_a / logp_p             float32, the same shapes (logp=True)
        values_a    [T + 1, E, n]   values_p [T + 1, E]  (values=True); row T is the bootstrap value: finish()
        slots       int32 [E]       the counters

    THE INVARIANT: exactly one store() per environment step, between the policy and Backend.step -- the store's ring and
    the reward log's ring advance one slot each per step and stay aligned only then.  After T steps (or any multiple)
    slot t holds time t.  `done` at step t means the episode ended there; under auto-reset slot t + 1 holds the restarted
    episode's first observation, and aie_gae does not carry value or advantage across that boundary."""

    def __init__(self, env, T, observations=("obs_a_flat", "obs_p_flat"), logp=True, values=True):
        import torch

        be = env.backend
        if be.host_components:
            raise NotImplementedError("Trajectory: the environment has host components (%s); their hooks run between launches "
                                      "issued from Python, not inside a captured iteration" % ", ".join(be.host_components))
        if getattr(be, "reward_log", None) is not None:
            raise RuntimeError("Trajectory: the backend already has a reward log (sharding.RewardLogGather owns it); a "
                               "trajectory installs its own of exactly T slots")
        self.env, self.be, self.T = env, be, int(T)
        if self.T < 1:
            raise ValueError("Trajectory: T >= 1")
        T, E, n, dev = self.T, be.E, be.n, be.device
        t = be.tensors
        self.has_logp, self.has_values = bool(logp), bool(values)
        self.obs = {name: torch.zeros((T,) + tuple(t[name].shape), dtype=t[name].dtype, device=dev) for name in observations}
        ma, mp = t["obs_a_action_mask"], t["obs_p_action_mask"]
        if ma.dtype != torch.float32 or mp.dtype != torch.float32:
            raise NotImplementedError("Trajectory: float32 action masks")
        from . import _cabi

        self._mask_rows = 0
        if int(be.cfg.scenario) == _cabi.SCN_COVID:  # the arena's collated [E, 1 + levels, n] -> [E, n, 1 + levels]
            self._mask_rows = int(ma.shape[1])
            self.masks_a = torch.zeros((T, E, ma.shape[2], ma.shape[1]), dtype=torch.float32, device=dev)
        else:
            self.masks_a = torch.zeros((T,) + tuple(ma.shape), dtype=torch.float32, device=dev)
        self.masks_p = torch.zeros((T,) + tuple(mp.shape), dtype=torch.float32, device=dev)
        aa, ap = be._action_buffers(0)
        self.actions_a = torch.zeros((T,) + tuple(aa.shape), dtype=torch.int32, device=dev)
        self.actions_p = torch.zeros((T,) + tuple(ap.shape), dtype=torch.int32, device=dev)
        self.logp_a = self.logp_p = self.values_a = self.values_p = None
        if self.has_logp:
            self.logp_a = torch.zeros((T,) + tuple(aa.shape), dtype=torch.float32, device=dev)
            self.logp_p = torch.zeros((T,) + tuple(ap.shape), dtype=torch.float32, device=dev)
        if self.has_values:
            self.values_a = torch.zeros((T + 1, E, n), dtype=torch.float32, device=dev)
            self.values_p = torch.zeros((T + 1, E), dtype=torch.float32, device=dev)
        self.slots = torch.zeros(E, dtype=torch.int32, device=dev)
        self.log = be.set_reward_log(T)
        seg = be.trajectory_segment
        self._fixed = [seg(t[name], self.obs[name]) for name in observations]
        self._fixed.append(seg(ma, self.masks_a, transpose_rows=self._mask_rows))
        self._fixed.append(seg(mp, self.masks_p))
        if len(self._fixed) + 2 + 2 * self.has_logp + 2 * self.has_values > _cabi.TRAJ_MAX_SEGMENTS:
            raise ValueError("Trajectory: more tensors than one store launch takes (%d segments)" % _cabi.TRAJ_MAX_SEGMENTS)

    def store(self, actions_a, actions_p, logp_a=None, logp_p=None, values_a=None, values_p=None):
        """ONE aie_trajectory_store launch on the current stream: the observations and masks as they stand, the given
        actions and -- where the trajectory keeps them -- logp and values go to the replicas' next slot, and the counters
        advance.  Call it between the policy and Backend.step, exactly once per environment step (see the class)."""
        be, E = self.be, self.be.E
        segs = list(self._fixed)
        segs.append(be.trajectory_segment(actions_a.view(self.actions_a.shape[1:]), self.actions_a))
        segs.append(be.trajectory_segment(actions_p.view(self.actions_p.shape[1:]), self.actions_p))
        for have, pairs, what in ((self.has_logp, ((logp_a, self.logp_a), (logp_p, self.logp_p)), "logp"),
                                  (self.has_values, ((values_a, self.values_a), (values_p, self.values_p)), "values")):
            if have:
                for src, dst in pairs:
                    if src is None:
                        raise ValueError("Trajectory.store: this trajectory keeps %s: pass both tensors" % what)
                    segs.append(be.trajectory_segment(src.view((E,) + tuple(dst.shape[2:])), dst[: self.T]))
        be.trajectory_store(segs, self.T, self.slots)

    def rewind(self):
        """The next store -- and the next step's rewards -- go to slot 0 again.  Outside capture (it zeroes the counters and
        restarts the reward log, which waits for the device)."""
        self.slots.zero_()
        self.be.rewind_reward_log()

    def finish(self, values_a, values_p):
        """Row T of the values: the bootstrap value of the observation behind the fragment's last step."""
        if not self.has_values:
            raise ValueError("Trajectory.finish: this trajectory keeps no values")
        self.values_a[self.T].copy_(values_a.view(self.values_a.shape[1:]))
        self.values_p[self.T].copy_(values_p.view(self.values_p.shape[1:]))

    def advantages(self, gamma=0.998, lam=0.98):
        """(adv_a [T, E, n], adv_p [T, E], ret_a, ret_p): aie_gae on the reward log and the stored values, one launch.
        Call it after T (or a multiple of T) steps since rewind(), and after finish()."""
        if not self.has_values:
            raise ValueError("Trajectory.advantages: this trajectory keeps no values")
        return self.be.gae(self.T, self.log, self.values_a, self.values_p, gamma, lam)

    def flat(self):
        """Everything as [T * E, ...] views (values: rows 0 .. T - 1), ready for rollout.masked_logp_entropy with B = T * E."""
        out = {"obs": {k: v.flatten(0, 1) for k, v in self.obs.items()}}
        for k in ("masks_a", "masks_p", "actions_a", "actions_p", "logp_a", "logp_p"):
            v = getattr(self, k)
            out[k] = None if v is None else v.flatten(0, 1)
        out["values_a"] = None if self.values_a is None else self.values_a[: self.T].flatten(0, 1)
        out["values_p"] = None if self.values_p is None else self.values_p[: self.T].flatten(0, 1)
        out["done"] = self.log[..., -1].flatten(0, 1)
        return out

    def ppo_batch(self, adv_a, adv_p, ret_a, ret_p):
        """The stored operands of rollout.ppo_loss / Backend.ppo_loss as [T * E, ...] views (nothing is copied): masks_*,
        actions_*, logp_old_* (the stored logp), values_old_* (the stored values, rows 0 .. T - 1), adv_* and returns_*
        (what advantages() returned, or the caller's own of those shapes).  A minibatch is an int32 index into its rows."""
        if not (self.has_logp and self.has_values):
            raise ValueError("Trajectory.ppo_batch: this trajectory keeps no logp or no values")
        T, E, n = self.T, self.be.E, self.be.n
        out = {}
        for who, adv, ret, shape in (("a", adv_a, ret_a, (T, E, n)), ("p", adv_p, ret_p, (T, E))):
            for name, t in (("adv_", adv), ("returns_", ret)):
                if tuple(t.shape) != shape or not t.is_contiguous():
                    raise ValueError("Trajectory.ppo_batch: %s%s must be a contiguous tensor of shape %s" % (name, who, shape))
                out[name + who] = t.flatten(0, 1)
            out["masks_" + who] = getattr(self, "masks_" + who).flatten(0, 1)
            out["actions_" + who] = getattr(self, "actions_" + who).flatten(0, 1)
            out["logp_old_" + who] = getattr(self, "logp_" + who).flatten(0, 1)
            out["values_old_" + who] = getattr(self, "values_" + who)[:T].flatten(0, 1)
        return out


def _masked_categorical():
    """The autograd Function, built at first use (torch is imported lazily everywhere in this package)."""
    global _MaskedCategorical
    if _MaskedCategorical is not None:
        return _MaskedCategorical
    import torch

    class MaskedCategorical(torch.autograd.Function):
        """log pi(a|s) and entropy of stored actions under stored masks, differentiable in the logits: forward =
        aie_policy_evaluate, backward = aie_policy_evaluate_backward (one launch each; the sampler's own float32
        arithmetic, so the logp of an action evaluated under the logits and masks it was sampled from IS the logp
        aie_sample_policy_actions_logp returned).  apply(be, logits_a, logits_p, masks_a, masks_p, actions_a, actions_p)
        -> (logp_a, logp_p, entropy_a, entropy_p); gradients flow to the logits only.  Either actor class may be None."""

        @staticmethod
        def forward(ctx, be, logits_a, logits_p, masks_a, masks_p, actions_a, actions_p):
            ctx.be = be
            ctx.has = (logits_a is not None, logits_p is not None)
            ctx.shapes = (None if logits_a is None else logits_a.shape, None if logits_p is None else logits_p.shape)
            la = None if logits_a is None else logits_a.detach()
            lp = None if logits_p is None else logits_p.detach()
            ctx.operands = (la, lp, masks_a, masks_p, actions_a, actions_p)
            out = be.policy_evaluate(la, lp, masks_a, masks_p, actions_a, actions_p)
            return tuple(out)

        @staticmethod
        def backward(ctx, g_logp_a, g_logp_p, g_ent_a, g_ent_p):
            ga, gp = ctx.be.policy_evaluate_backward(*ctx.operands, g_logp_a=g_logp_a, g_logp_p=g_logp_p,
                                                     g_entropy_a=g_ent_a, g_entropy_p=g_ent_p)
            if ga is not None:
                ga = ga.view(ctx.shapes[0])
            if gp is not None:
                gp = gp.view(ctx.shapes[1])
            return None, ga, gp, None, None, None, None

    _MaskedCategorical = MaskedCategorical
    return MaskedCategorical


_MaskedCategorical = None


def _ppo_loss_function():
    """The autograd Function of ppo_loss, built at first use."""
    global _PPOLoss
    if _PPOLoss is not None:
        return _PPOLoss
    import torch

    class PPOLoss(torch.autograd.Function):
        """Both classes' PPO loss, differentiable in the logits and the values: forward = ONE Backend.ppo_loss call
        (aie_ppo_loss: two launches, forward and backward together), which already leaves the gradients of the two
        losses; backward multiplies them by the incoming scalars.  apply(be, logits_a, logits_p, values_a, values_p, batch,
        index, coefficients, coeffs_p, adv_moments) -> (loss_a, loss_p, stats_a, stats_p)."""

        @staticmethod
        def forward(ctx, be, logits_a, logits_p, values_a, values_p, batch, index, coefs, coeffs_p, adv_moments):
            out_a, out_p = be.ppo_loss(logits_a, logits_p, values_a, values_p, batch, index=index, coeffs_p=coeffs_p,
                                       adv_moments=adv_moments, **coefs)
            ctx.grads = []
            res = []
            for out, lg, val in ((out_a, logits_a, values_a), (out_p, logits_p, values_p)):
                if out is None:
                    ctx.grads.append((None, None))
                    res.append((None, None))
                    continue
                stats, g, gv = out
                ctx.grads.append((g.view(lg.shape), None if gv is None else gv.view(val.shape)))
                res.append((stats[0].clone(), stats))
            stats = [r[1] for r in res if r[1] is not None]
            ctx.mark_non_differentiable(*stats)
            return res[0][0], res[1][0], res[0][1], res[1][1]

        @staticmethod
        @torch.autograd.function.once_differentiable  # (the stored gradients are constants: a double backward raises)
        def backward(ctx, g_loss_a, g_loss_p, _sa, _sp):
            out = []
            for (g, gv), up in zip(ctx.grads, (g_loss_a, g_loss_p)):
                out.append((None if g is None or up is None else g * up, None if gv is None or up is None else gv * up))
            return None, out[0][0], out[1][0], out[0][1], out[1][1], None, None, None, None, None

    _PPOLoss = PPOLoss
    return PPOLoss


_PPOLoss = None


def ppo_loss(be, logits_a, logits_p, values_a, values_p, batch, index=None, clip=0.3, vf_clip=50.0, vf_coef=0.05, ent_coef=0.025,
             coeffs_p=None, adv_moments=None):
    """(loss_a, loss_p, stats_a, stats_p): the PPO loss of both actor classes -- the clipped surrogate over the joint
    log-probability of an actor's action slots, the clipped value loss, the entropy bonus -- as 0-dim tensors that are
    differentiable in the logits and the values, and each class's statistics (float32 [8]: loss, policy, value, entropy,
    kl, clip fraction, skipped actors, max |log-ratio|; include/aie.h).  One library call of two launches computes the
    losses AND their gradients, whatever the batch size; `batch` holds the stored operands (Trajectory.ppo_batch()) and
    `index` (int32 [B] on the device, or None) picks the minibatch's rows out of them without a copy.  Operands and
    coefficients: Backend.ppo_loss.  A class whose logits are None gives (None, None)."""
    coefs = dict(clip=clip, vf_clip=vf_clip, vf_coef=vf_coef, ent_coef=ent_coef)
    return _ppo_loss_function().apply(be, logits_a, logits_p, values_a, values_p, batch, index, coefs, coeffs_p, adv_moments)


def _policy_mlp_function():
    """The autograd Function of policy_mlp, built at first use."""
    global _PolicyMLP
    if _PolicyMLP is not None:
        return _PolicyMLP
    import torch

    class PolicyMLP(torch.autograd.Function):
        """Both classes' policy network, differentiable in its weights: forward = ONE Backend.policy_mlp_forward call,
        backward = ONE Backend.policy_mlp_backward call (three launches).  apply(be, x_a, x_p, names_a, names_p, *weights)
        -> (logits_a, logits_p, value_a, value_p); names_*: the keys of the class's weights among `weights`, in order."""

        @staticmethod
        def forward(ctx, be, x_a, x_p, names_a, names_p, *weights):
            wa = dict(zip(names_a, weights[:len(names_a)]))
            wp = dict(zip(names_p, weights[len(names_a):]))
            out = be.policy_mlp_forward(x_a, x_p, wa if x_a is not None else None, wp if x_p is not None else None)
            ctx.be, ctx.names = be, (names_a, names_p)
            ctx.has_x = (x_a is not None, x_p is not None)
            ctx.save_for_backward(*[t for t in (x_a, x_p) if t is not None], *weights)
            return out

        @staticmethod
        @torch.autograd.function.once_differentiable  # (one library call, not a graph of torch operations)
        def backward(ctx, g_la, g_lp, g_va, g_vp):
            saved = list(ctx.saved_tensors)
            x_a = saved.pop(0) if ctx.has_x[0] else None
            x_p = saved.pop(0) if ctx.has_x[1] else None
            names_a, names_p = ctx.names
            wa, wp = dict(zip(names_a, saved[:len(names_a)])), dict(zip(names_p, saved[len(names_a):]))
            c = lambda g: None if g is None else g.contiguous()  # noqa: E731  (a missing one arrives as zeros)
            ga, gp = ctx.be.policy_mlp_backward(x_a, x_p, wa, wp, c(g_la), c(g_lp), c(g_va) if "wv" in wa else None,
                                                c(g_vp) if "wv" in wp else None)
            grads = [ga[k] if ga is not None else None for k in names_a] + [gp[k] if gp is not None else None for k in names_p]
            return (None,) * 5 + tuple(grads)

    _PolicyMLP = PolicyMLP
    return PolicyMLP


_PolicyMLP = None


def policy_mlp(be, x_a, x_p, weights_a, weights_p):
    """(logits_a, logits_p, value_a, value_p) of Backend.policy_mlp_forward -- the same operands, the same bits -- as
    tensors that are differentiable in the sixteen weight tensors (those with requires_grad): backward is ONE
    Backend.policy_mlp_backward call in the forward's float32 chains, bit-reproducible (include/aie.h states the
    arithmetic).  Nothing flows to the observations; an output that takes no part in the loss counts as a zero gradient.
    With ppo_loss on the outputs, loss.backward() fills .grad of [in, out] weight tensors an in-place optimizer updates
    where the next forward -- eager or replayed -- reads them: no mlp_weights.refresh()."""
    names, flat = [], []
    for x, w in ((x_a, weights_a), (x_p, weights_p)):
        get = (lambda k: None) if x is None else w.get if hasattr(w, "get") else (lambda k, w=w: getattr(w, k, None))
        present = tuple(k for k in mlp_weights.NAMES if get(k) is not None)
        names.append(present)
        flat.extend(get(k) for k in present)
    return _policy_mlp_function().apply(be, x_a, x_p, names[0], names[1], *flat)


def _policy_conv_mlp_function():
    """The autograd Function of policy_conv_mlp, built at first use."""
    global _PolicyConvMLP
    if _PolicyConvMLP is not None:
        return _PolicyConvMLP
    import torch

    class PolicyConvMLP(torch.autograd.Function):
        """The agents' convolutional encoder in front of both classes' policy network, differentiable in all weights:
        forward = Backend.policy_conv_forward, then Backend.policy_mlp_forward; backward = Backend.policy_mlp_backward,
        Backend.policy_mlp_input_grad, Backend.policy_conv_backward, in that order.
        apply(be, map, idx, flat, x_p, names_c, names_a, names_p, *weights) -> (logits_a, logits_p, value_a, value_p)."""

        @staticmethod
        def forward(ctx, be, map_, idx, flat, x_p, names_c, names_a, names_p, *weights):
            nc, na = len(names_c), len(names_a)
            wc, wa, wp = dict(zip(names_c, weights[:nc])), dict(zip(names_a, weights[nc:nc + na])), dict(zip(names_p, weights[nc + na:]))
            x_cat = be.policy_conv_forward(map_, idx, flat, wc)
            out = be.policy_mlp_forward(x_cat, x_p, wa, wp if x_p is not None else None)
            ctx.be, ctx.names = be, (names_c, names_a, names_p)
            ctx.has_p = x_p is not None
            ctx.NF = x_cat.shape[1] - (flat.shape[-1] if flat is not None else 0)
            ctx.save_for_backward(map_, idx, x_cat, *([x_p] if x_p is not None else []), *weights)
            return out

        @staticmethod
        @torch.autograd.function.once_differentiable  # (library calls, not a graph of torch operations)
        def backward(ctx, g_la, g_lp, g_va, g_vp):
            saved = list(ctx.saved_tensors)
            map_, idx, x_cat = saved[:3]
            del saved[:3]
            x_p = saved.pop(0) if ctx.has_p else None
            names_c, names_a, names_p = ctx.names
            nc, na = len(names_c), len(names_a)
            wc, wa, wp = dict(zip(names_c, saved[:nc])), dict(zip(names_a, saved[nc:nc + na])), dict(zip(names_p, saved[nc + na:]))
            c = lambda g: None if g is None else g.contiguous()  # noqa: E731  (a missing one arrives as zeros)
            be = ctx.be
            ga, gp = be.policy_mlp_backward(x_cat, x_p, wa, wp, c(g_la), c(g_lp), c(g_va) if "wv" in wa else None,
                                            c(g_vp) if "wv" in wp else None)
            g_x, _ = be.policy_mlp_input_grad(ncols_a=ctx.NF)
            gc = be.policy_conv_backward(map_, idx, wc, g_x)
            grads = [gc[k] for k in names_c] + [ga[k] for k in names_a] + [gp[k] if gp is not None else None for k in names_p]
            return (None,) * 8 + tuple(grads)

    _PolicyConvMLP = PolicyConvMLP
    return PolicyConvMLP


_PolicyConvMLP = None
CONV_NAMES = ("emb", "w1", "b1", "w2", "b2")  # the encoder's tensors: Backend.policy_conv_forward's conv_weights


def policy_conv_mlp(be, map, idx, flat, conv_weights, x_p, weights_a, weights_p):  # noqa: A002
    """policy_mlp with the convolutional encoder of the egocentric crop in front of the agents' network: (logits_a, logits_p,
    value_a, value_p), where the agents' rows are Backend.policy_conv_forward(map, idx, flat, conv_weights) -- the crop's 128
    features, then the flat observation -- through weights_a (w1 [NF + F_flat, H]), and the planner's are x_p through weights_p
    as before (x_p None: left out).  Differentiable in the encoder's five and the networks' sixteen tensors: backward runs,
    in order, Backend.policy_mlp_backward, Backend.policy_mlp_input_grad and Backend.policy_conv_backward -- seven launches,
    float32 chains in fixed orders, bit-reproducible (include/aie.h states the arithmetic).  Nothing flows to the observations."""
    getc = conv_weights.get if hasattr(conv_weights, "get") else (lambda k: getattr(conv_weights, k, None))
    names, flat_w = [CONV_NAMES], [getc(k) for k in CONV_NAMES]
    for x, w in ((map, weights_a), (x_p, weights_p)):
        get = (lambda k: None) if x is None else w.get if hasattr(w, "get") else (lambda k, w=w: getattr(w, k, None))
        present = tuple(k for k in mlp_weights.NAMES if get(k) is not None)
        names.append(present)
        flat_w.extend(get(k) for k in present)
    return _policy_conv_mlp_function().apply(be, map, idx, flat, x_p, names[0], names[1], names[2], *flat_w)


class Adam:
    """Adam under a gradient-norm clip for the two actor classes' parameters, ONE library call of two launches per step
    (Backend.adam_step, aie_adam_step) -- the optimizer the reference's tutorials train with (lr 0.0003, grad_clip 10), one
    parameter group and one norm per class.  params_a / params_p: a mapping of tensors (a MaskedMLPPolicy's weights_a /
    weights_p) or a sequence of them, at most 16 per class, contiguous float32 device tensors that are updated where they
    lie (the next policy_mlp_forward, eager or replayed, reads the new values); None leaves a class out.  This object owns
    the moments m and v, each class's state (int64 [4]: the step count t, then the bits of beta1^t and beta2^t) and
    statistics, the learning rate (ONE float32 on the device for both classes) and the workspace; nothing is allocated
    after the constructor.  max_norm <= 0: no clipping.
    step(grads=None): grads = (grads_a, grads_p), shaped like the parameters (mappings with their keys, or sequences in
    their order: policy_mlp_backward's dicts); None reads each parameter's .grad (for a view, such as MaskedMLPPolicy's
    value column, its base's).  Gradients are used where they lie -- contiguous float32 device tensors, never converted --
    and are neither modified, zeroed nor freed.  Captured in a graph, a replay advances t and reads the learning rate
    anew: set_lr(x) between replays is a schedule.  A class whose gradient norm is not finite is skipped (stats()[..][3]
    == 1): its weights, moments and step count stay.  The arithmetic is include/aie.h's: two runs give the same bits."""

    def __init__(self, be, params_a, params_p, lr=3e-4, betas=(0.9, 0.999), eps=1e-8, max_norm=10.0):
        import torch

        from . import _cabi

        self.be = be
        self.betas, self.eps, self.max_norm = (float(betas[0]), float(betas[1])), float(eps), float(max_norm)
        self.lr = torch.full((1,), float(lr), dtype=torch.float32, device=be.device)
        self.groups = []
        need = 0
        for params in (params_a, params_p):
            if params is None:
                self.groups.append(None)
                continue
            keys = list(params.keys()) if hasattr(params, "keys") else None
            ps = [params[k] for k in keys] if keys is not None else list(params)
            if not 1 <= len(ps) <= _cabi.OPT_MAX_TENSORS:
                raise ValueError("Adam: a class has 1 .. %d parameter tensors (%d given)" % (_cabi.OPT_MAX_TENSORS, len(ps)))
            for p in ps:
                if not isinstance(p, torch.Tensor) or p.dtype != torch.float32 or p.device != be.device or not p.is_contiguous() \
                        or p.numel() < 1:
                    raise ValueError("Adam: parameters are contiguous float32 tensors on the backend's device")
            f = dict(dtype=torch.float32, device=be.device)
            self.groups.append(dict(
                keys=keys, params=[p.detach() for p in ps], src=ps,
                m=[torch.zeros(p.numel(), **f) for p in ps], v=[torch.zeros(p.numel(), **f) for p in ps],
                state=torch.zeros(_cabi.OPT_STATE_BYTES // 8, dtype=torch.int64, device=be.device),
                stats=torch.zeros(_cabi.OPT_N_STATS, **f)))
            need += 4 + sum(-(-p.numel() // _cabi.OPT_CHUNK) for p in ps)  # float64 words: include/aie.h's formula
        if need == 0:
            raise ValueError("Adam: no parameters")
        self.workspace = torch.zeros(need, dtype=torch.float64, device=be.device)

    @staticmethod
    def _grad_of(p):
        g = p.grad
        base = getattr(p, "_base", None)
        if g is None and base is not None and base.numel() == p.numel() and base.is_contiguous():
            g = base.grad
        if g is None:
            raise ValueError("Adam.step: a parameter has no .grad (run backward first, or pass grads=)")
        return g

    def step(self, grads=None):
        """One step of both classes: one Backend.adam_step call on the current stream."""
        descs = []
        for c, G in enumerate(self.groups):
            if G is None:
                descs.append(None)
                continue
            if grads is None:
                gs = [self._grad_of(p) for p in G["src"]]
            else:
                given = grads[c]
                gs = [given[k] for k in G["keys"]] if G["keys"] is not None and hasattr(given, "keys") else list(given)
            if len(gs) != len(G["params"]):
                raise ValueError("Adam.step: %d gradients for %d parameters" % (len(gs), len(G["params"])))
            descs.append(self.be.adam_group(zip(G["params"], gs, G["m"], G["v"]), self.lr, G["state"], G["stats"],
                                            betas=self.betas, eps=self.eps, max_norm=self.max_norm))
        self.be.adam_step(descs[0], descs[1], self.workspace)

    def set_lr(self, lr):
        """Fills the learning rate's device scalar: seen by the next step, or the next replay of a captured one."""
        self.lr.fill_(float(lr))

    def stats(self):
        """(stats_a, stats_p): float32 [4] device tensors -- the gradient norm before clipping, the clip coefficient, the
        step count after the last call, 1 if that call skipped the class -- or None for a class left out."""
        return tuple(None if G is None else G["stats"] for G in self.groups)

    def steps(self):
        """(t_a, t_p): each class's step count as a 0-dim int64 device tensor (a view of its state), or None."""
        return tuple(None if G is None else G["state"][0] for G in self.groups)


def __getattr__(name):  # rollout.MaskedCategorical, rollout.PPOLoss, rollout.PolicyMLP: the classes, made when first asked for
    if name == "MaskedCategorical":
        return _masked_categorical()
    if name == "PPOLoss":
        return _ppo_loss_function()
    if name == "PolicyMLP":
        return _policy_mlp_function()
    if name == "PolicyConvMLP":
        return _policy_conv_mlp_function()
    raise AttributeError(name)


def masked_logp_entropy(be, logits_a, logits_p, masks_a, masks_p, actions_a, actions_p):
    """(logp_a, logp_p, entropy_a, entropy_p) of the stored actions under the stored masks for the given logits (layouts:
    Backend.sample_policy_actions / Backend.action_masks, any batch size B in place of E; masks None = the environment's
    current masks, B = E), differentiable in the logits: what a PPO / A2C loss is built from.  Two launches per
    training step in all (forward, backward) where the torch formulation (masked_fill, log_softmax, gather, the entropy
    sum and their autograd twins) takes 10 - 15 per actor class -- and the distribution is the sampler's, to the bit."""
    return _masked_categorical().apply(be, logits_a, logits_p, masks_a, masks_p, actions_a, actions_p)


class mlp_weights:
    """The [in, out] float32 tensors Backend.policy_mlp_forward takes, made from three torch.nn.Linear (plus an optional
    value Linear of one output) -- or from their (weight, bias) tensor pairs in Linear's [out, in] layout: transposed
    COPIES on the module's device, so refresh() must be called after every optimizer step (it copies in place: the
    tensors keep their addresses, a captured launch sees the new values on its next replay).  A trainer that keeps its
    parameters as [in, out] needs none of this: it hands a dict of its own tensors to policy_mlp_forward, no copy.
    Attributes (and get(name)): w1, b1, w2, b2, w3, b3, wv, bv (the last two None without a value layer)."""

    NAMES = ("w1", "b1", "w2", "b2", "w3", "b3", "wv", "bv")

    def __init__(self, l1, l2, l3, value=None):
        import torch

        def pair(m):
            return (m.weight, m.bias) if hasattr(m, "weight") else tuple(m)

        self._src = [pair(m) for m in (l1, l2, l3)] + ([pair(value)] if value is not None else [])
        for w, b in self._src:
            if w.dim() != 2 or b is None or w.dtype != torch.float32:
                raise ValueError("mlp_weights: float32 Linear layers with a bias")
        if value is not None and self._src[3][0].shape[0] != 1:
            raise ValueError("mlp_weights: the value layer has one output")
        self.wv = self.bv = None
        with torch.no_grad():
            for i, (w, b) in enumerate(self._src):
                wt = torch.empty((w.shape[1], w.shape[0]), dtype=w.dtype, device=w.device).copy_(w.detach().t())  # (never a view)
                name = ("1", "2", "3", "v")[i]
                setattr(self, "w" + name, wt.view(-1) if name == "v" else wt)
                setattr(self, "b" + name, b.detach().clone().view(-1))

    def get(self, name, default=None):
        return getattr(self, name, default) if name in self.NAMES else default

    def refresh(self):
        """Copies the modules' current parameters into the same tensors, in place."""
        import torch

        with torch.no_grad():
            for (w, b), name in zip(self._src, ("1", "2", "3", "v")):
                getattr(self, "w" + name).view(w.shape[1], w.shape[0]).copy_(w.detach().t())
                getattr(self, "b" + name).copy_(b.detach().view(-1))
        return self


class MaskedMLPPolicy:
    """A small policy network of the shape the reference's trainers use on the flat observations (fully connected
    trunk, one categorical head per action subspace, `action_mask` applied to the logits: base_env.py:141-145,
    tutorials/rllib/env_wrapper.py:50-211) with random-init weights: enough to put a real policy's launches between the
    environment steps.  The network is torch (three GEMMs with fused bias per actor class, two ReLUs); masking and
    sampling -- what every trainer does with its logits -- is ONE launch of the library (aie_sample_policy_actions:
    inverse-CDF sampling under the action masks in float32, fixed operation order, the draw index a record field, so the
    loop can be captured).  record_logp=True: the same launch also fills `logp_a` / `logp_p` (float32, the action
    buffers' shapes) with log pi(a|s) of every pick, in place -- a trainer copies them into its trajectory with the
    actions and Backend.action_masks().
    `sampler="torch"` keeps the round-4 formulation (Gumbel noise, masked_fill and argmax as ~15 elementwise launches per
    actor class) for comparison.
    value_head=True: one more output column per actor class (the critic), written in place on every call into the fixed
    float32 tensors `value_a` [E, n] and `value_p` [E] -- what rollout.Trajectory stores beside the actions.  Its weights
    are drawn behind the six layers', so the policy's own weights do not depend on it.
    network="library": logits() is ONE Backend.policy_mlp_forward call (aie_policy_mlp_forward: both classes' three
    layers and value columns in one launch, float32, every output one ascending fmaf chain from its bias) that reads the
    arena's observations and this object's weight tensors where they lie and writes the fixed buffers `logits_a` /
    `logits_p` and `value_a` / `value_p` in place; a call of the policy is then two launches, the network and the sampler.
    float32 only.  evaluate(x_a, x_p) is the same network as an autograd function (rollout.policy_mlp) on the same
    weight tensors: what a PPO update differentiates.  The default "torch" path is unchanged.
    spatial=True (network="library" only): the agents also see their egocentric crop -- obs_a_world-map and
    obs_a_world-idx_map through the library's convolutional encoder (Backend.policy_conv_forward: an embedding of emb_dim
    per index plane over emb_vocab entries, two 3x3 stride-2 convolutions, 128 features on the 11 x 11 crop; the network of
    the reference's tutorials), concatenated in front of the flat observation in the fixed buffer `x_cat` [E * n, NF + FA].
    logits() is then two launches, encoder and MLP; evaluate((map, idx, flat), x_p) is the differentiable form
    (rollout.policy_conv_mlp).  The encoder's five tensors (`conv_weights`) and the NF feature rows of the agents' first
    layer are drawn behind all other weights, so a seed gives the weights it gave before, and spatial=False is unchanged.
    `params_a` / `params_p`: every trainable tensor of a class, by name (the agents' 13 with the encoder's as conv_*), what
    rollout.Adam takes."""

    def __init__(self, be, hidden=128, seed=0, dtype=None, sampler="library", sample_seed=1234, record_logp=False,
                 value_head=False, network="torch", spatial=False, emb_vocab=100, emb_dim=4):
        import torch

        self.torch = torch
        self.be = be
        t = be.tensors
        g = torch.Generator(device="cpu").manual_seed(seed)
        dev = be.device
        dtype = dtype or torch.float32
        self.dtype = dtype
        FA = t["obs_a_flat"].shape[-1]
        MA = t["obs_a_action_mask"].shape[-1]
        FP = t["obs_p_flat"].shape[-1]
        MP = t["obs_p_action_mask"].shape[-1]

        def lin(i, o):
            return (torch.randn(i, o, generator=g) / i ** 0.5).to(dev, dtype), torch.zeros(o, device=dev, dtype=dtype)

        self.wa1, self.ba1 = lin(FA, hidden)
        self.wa2, self.ba2 = lin(hidden, hidden)
        self.wa3, self.ba3 = lin(hidden, MA)
        self.wp1, self.bp1 = lin(FP, hidden)
        self.wp2, self.bp2 = lin(hidden, hidden)
        self.wp3, self.bp3 = lin(hidden, MP)
        self.MA, self.MP = MA, MP
        self.value_head = bool(value_head)
        self.value_a = self.value_p = None
        if self.value_head:
            self.wav, self.bav = lin(hidden, 1)
            self.wpv, self.bpv = lin(hidden, 1)
            self.value_a = torch.zeros((be.E, be.n), dtype=torch.float32, device=dev)
            self.value_p = torch.zeros((be.E,), dtype=torch.float32, device=dev)
        cfg = be.cfg
        self.multi_a = bool(cfg.multi_action_mode_agents)
        self.multi_p = bool(cfg.multi_action_mode_planner)
        self.p_width = be._act_p_width()
        assert sampler in ("library", "torch")
        self.sampler = sampler
        self.sample_seed = int(sample_seed)
        if self.multi_a and sampler == "torch":
            raise NotImplementedError("MaskedMLPPolicy(sampler='torch'): single-action agents (the BASELINE configurations)")
        self.record_logp = bool(record_logp)
        self.logp_a = self.logp_p = None
        if self.record_logp:
            if sampler != "library":
                raise NotImplementedError("MaskedMLPPolicy(record_logp=True): the library's sampler")
            aa, ap = be._action_buffers(0)
            self.logp_a = torch.zeros(aa.shape, dtype=torch.float32, device=dev)
            self.logp_p = torch.zeros(ap.shape, dtype=torch.float32, device=dev)
        if network not in ("torch", "library"):
            raise ValueError("MaskedMLPPolicy: network is 'torch' or 'library'")
        self.network = network
        if network == "library":
            if dtype != torch.float32:
                raise ValueError("MaskedMLPPolicy(network='library'): float32 weights (dtype %s given)" % dtype)
            names = ("w1", "b1", "w2", "b2", "w3", "b3")
            self.weights_a = dict(zip(names, (self.wa1, self.ba1, self.wa2, self.ba2, self.wa3, self.ba3)))
            self.weights_p = dict(zip(names, (self.wp1, self.bp1, self.wp2, self.bp2, self.wp3, self.bp3)))
            if self.value_head:  # (views of the [hidden, 1] columns: an in-place update reaches them)
                self.weights_a.update(wv=self.wav.view(-1), bv=self.bav)
                self.weights_p.update(wv=self.wpv.view(-1), bv=self.bpv)
            self.logits_a = torch.zeros((be.E * be.n, MA), dtype=torch.float32, device=dev)
            self.logits_p = torch.zeros((be.E, MP), dtype=torch.float32, device=dev)
            self.params_a, self.params_p = dict(self.weights_a), dict(self.weights_p)
        self.spatial = bool(spatial)
        if self.spatial:
            if network != "library":
                raise ValueError("MaskedMLPPolicy(spatial=True): network='library'")
            from . import _cabi

            if "obs_a_world-map" not in t or "obs_a_world-idx_map" not in t:
                raise ValueError("MaskedMLPPolicy(spatial=True): the scenario has no egocentric crop (obs_a_world-map)")
            C_map, h, w = (int(v) for v in t["obs_a_world-map"].shape[-3:])
            C = C_map + 2 * int(emb_dim)
            oh1, ow1 = (h - 3) // 2 + 1, (w - 3) // 2 + 1
            self.NF = ((oh1 - 3) // 2 + 1) * ((ow1 - 3) // 2 + 1) * _cabi.CONV_F2
            # drawn behind every weight above: the encoder's tensors, then the first layer's rows for its features
            emb = torch.randn(int(emb_vocab), int(emb_dim), generator=g).to(dev, dtype)
            cw1, cb1 = lin(9 * C, _cabi.CONV_F1)
            cw2, cb2 = lin(9 * _cabi.CONV_F1, _cabi.CONV_F2)
            self.conv_weights = dict(emb=emb, w1=cw1, b1=cb1, w2=cw2, b2=cb2)
            w_feat, _ = lin(self.NF, hidden)
            self.wa1 = torch.cat([w_feat, self.wa1], 0).contiguous()
            self.weights_a["w1"] = self.wa1
            self.params_a = dict(self.weights_a, **{"conv_" + k: v for k, v in self.conv_weights.items()})
            self.x_cat = torch.zeros((be.E * be.n, self.NF + FA), dtype=torch.float32, device=dev)
        self._fused_relu = None  # decided at the first call (outside any capture: GraphedStep warms the policy up first)
        self.counter = torch.zeros((), dtype=torch.float32, device=dev)
        if sampler == "torch":
            self.idx_a = torch.arange(be.E * be.n * MA, device=dev, dtype=torch.float32).view(be.E, be.n, MA)
            self.idx_p = torch.arange(be.E * MP, device=dev, dtype=torch.float32).view(be.E, MP)

    def _gumbel(self, idx, salt):
        torch = self.torch
        u = torch.frac(torch.sin(idx * 12.9898 + (self.counter + salt) * 78.233) * 43758.5453).abs_()
        u = u.clamp_(1e-6, 1.0 - 1e-6)
        return -torch.log(-torch.log(u))

    def _layer(self, b, x, w):
        """relu(x @ w + b): one launch where the BLAS library fuses the activation into the GEMM's epilogue
        (torch._addmm_activation), else the GEMM and an in-place ReLU."""
        torch = self.torch
        if self._fused_relu is None:
            self._fused_relu = False
            fn = getattr(torch, "_addmm_activation", None)
            if fn is not None:
                try:
                    got = fn(b, x, w, use_gelu=False)
                    self._fused_relu = bool(torch.allclose(got, torch.addmm(b, x, w).relu_(), rtol=1e-4, atol=1e-4))
                except Exception:
                    self._fused_relu = False
        if self._fused_relu:
            return torch._addmm_activation(b, x, w, use_gelu=False)
        return torch.addmm(b, x, w).relu_()

    def logits(self, tensors):
        """(agents' logits [E * n, MA], planner's logits [E, MP]) in the layout of the flattened action masks."""
        torch = self.torch
        if self.network == "library":
            xa, xp = tensors["obs_a_flat"], tensors["obs_p_flat"]
            if xa.dtype != torch.float32 or xp.dtype != torch.float32:
                raise ValueError("MaskedMLPPolicy(network='library'): float32 observations")
            if self.spatial:
                xa = self.be.policy_conv_forward(tensors["obs_a_world-map"], tensors["obs_a_world-idx_map"], xa, self.conv_weights,
                                                 out=self.x_cat)
            self.be.policy_mlp_forward(xa, xp, self.weights_a, self.weights_p,
                                       out=(self.logits_a, self.logits_p, self.value_a, self.value_p))
            return self.logits_a, self.logits_p
        xa = tensors["obs_a_flat"].to(self.dtype).reshape(-1, self.wa1.shape[0])
        h = self._layer(self.ba1, xa, self.wa1)
        h = self._layer(self.ba2, h, self.wa2)
        la = torch.addmm(self.ba3, h, self.wa3).float()
        if self.value_head:
            self.value_a.view(-1, 1).copy_(torch.addmm(self.bav, h, self.wav))
        xp = tensors["obs_p_flat"].to(self.dtype)
        h = self._layer(self.bp1, xp, self.wp1)
        h = self._layer(self.bp2, h, self.wp2)
        lp = torch.addmm(self.bp3, h, self.wp3).float()
        if self.value_head:
            self.value_p.view(-1, 1).copy_(torch.addmm(self.bpv, h, self.wpv))
        return la, lp

    def evaluate(self, x_a, x_p):
        """network="library": policy_mlp's (logits_a, logits_p, value_a, value_p) for the given observations (any batch
        size) on this object's own weight tensors, differentiable in those that require a gradient: with ppo_loss on
        them, backward() fills .grad of wa1 .. bpv, and an in-place optimizer step is what the next call, logits() or
        replay sees.  New tensors: the fixed buffers of logits() are not touched.  spatial=True: x_a is the triple
        (map, idx, flat) -- the crop's two tensors and the flat observation, stored copies included -- and the encoder's
        tensors take gradients too (rollout.policy_conv_mlp)."""
        if self.network != "library":
            raise NotImplementedError("MaskedMLPPolicy.evaluate: network='library'")
        wa, wp = dict(self.weights_a), dict(self.weights_p)
        if self.value_head:  # (views made now, so that a gradient reaches the [hidden, 1] columns)
            wa["wv"], wp["wv"] = self.wav.view(-1), self.wpv.view(-1)
        if self.spatial:
            map_, idx, flat = x_a
            return policy_conv_mlp(self.be, map_, idx, flat, self.conv_weights, x_p, wa, wp)
        return policy_mlp(self.be, x_a, x_p, wa, wp)

    def __call__(self, tensors, actions_a, actions_p):
        torch = self.torch
        la, lp = self.logits(tensors)
        if self.sampler == "library":
            if self.record_logp:
                self.be.sample_policy_actions(la, lp, self.sample_seed, out=(actions_a, actions_p, self.logp_a, self.logp_p), logp=True)
            else:
                self.be.sample_policy_actions(la, lp, self.sample_seed, out=(actions_a, actions_p))
            return
        la = la.view(self.be.E, self.be.n, self.MA) + self._gumbel(self.idx_a, 0.0)
        la = la.masked_fill(tensors["obs_a_action_mask"] < 0.5, -1e30)
        actions_a.view(self.be.E, self.be.n).copy_(la.argmax(-1))
        lp = lp + self._gumbel(self.idx_p, 0.5)
        lp = lp.masked_fill(tensors["obs_p_action_mask"] < 0.5, -1e30)
        if self.multi_p and self.p_width > 1:  # one categorical head per bracket: [E, width, 1 + rates]
            actions_p.copy_(lp.view(self.be.E, self.p_width, -1).argmax(-1))
        else:
            actions_p.view(self.be.E).copy_(lp.argmax(-1))
        self.counter += 1.0
