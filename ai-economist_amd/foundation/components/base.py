"""Base class for component specs (reference: F/base/base_component.py:16-375)."""
from ..registrar import Registry


class BaseComponent:
    name = ""
    component_type = None
    agent_subclasses = None
    required_entities = None
    comp_id = 0  # AIE_COMP_* in include/aie.h

    def __init__(self, n_agents, episode_length, inventory_scale=1):
        assert self.name
        assert isinstance(self.agent_subclasses, (tuple, list)) and self.agent_subclasses
        assert isinstance(self.required_entities, (tuple, list))
        assert isinstance(episode_length, int) and episode_length > 0
        self.n_agents = int(n_agents)
        self._episode_length = episode_length
        self._inventory_scale = float(inventory_scale)

    @property
    def episode_length(self):
        return int(self._episode_length)

    @property
    def inv_scale(self):
        return self._inventory_scale

    @property
    def shorthand(self):
        return self.name if self.component_type is None else self.component_type

    def get_n_actions(self, agent_cls_name):
        raise NotImplementedError

    def agent_state_fields(self):
        """{agent.state field the component adds (get_additional_state_fields): state tensor};
        used when the reference-shaped per-agent state is rebuilt (dense logs)."""
        return {}

    def fill_config(self, cfg):
        """Writes this component's kwargs into an AieConfig (ctypes)."""
        raise NotImplementedError


class BatchedComponent(BaseComponent):
    """A user's component whose dynamics are HOST code over the batch (round 6).

    The reference's component registry is open (F/base/base_component.py:378, F/base/registrar.py:48-66): anybody can
    subclass BaseComponent, register the class and list it in `components`.  The built-in components' dynamics are device
    kernels here, which a Python class cannot join -- but it can run BETWEEN launches.  A registered subclass of this class
    is placed in the component list like any other; the environment then steps through `aie_step_range` (include/aie.h):
    the built-in components ahead of it in one launch, then its `component_step(tensors)` as torch code on the zero-copy
    state tensors of all replicas at once, then the next stretch of built-ins, ... and the end of the step (regeneration,
    observations, masks, rewards) in the last launch.  Same order of effects as the reference's
    `for component in self._components: component.component_step()` (base_env.py:985-987).

        @foundation.components.add
        class CoinSubsidy(foundation.BatchedComponent):
            name = "CoinSubsidy"
            required_entities = ["Coin"]
            agent_subclasses = ["BasicMobileAgent"]

            def __init__(self, *args, amount=1.0, **kwargs):
                super().__init__(*args, **kwargs)
                self.amount = float(amount)

            def component_step(self, t):                    # t: {name: tensor [n_envs, ...]}, the arena's own memory
                t["inv_coin"] += self.amount

            def generate_observations(self, t):             # optional: {"a": {key: [n_envs, n_agents(, k)]}, "p": {key: [n_envs(, k)]}}
                return {"a": {"amount": t["inv_coin"].new_full(t["inv_coin"].shape, self.amount)}, "p": {}}

    What it can do: read and write every state tensor (`env.tensors`: inv_coin, inv_res, labor, loc_r / loc_c, stone /
    wood / house_owner, ... the names of include/aie.h's tensor table), add observations (they enter the flat vectors at
    their sorted-key position "<name>-<key>" exactly as the reference packs them, base_env.py:561-612, or appear under
    that key with flatten_observations=False), keep its own torch state, take part in reset (`additional_reset_steps`).
    What it cannot: own an ACTION subspace (`get_n_actions` must return None here -- a component that acts subclasses
    foundation.ActingComponent, below), draw from a replica's NumPy stream, run in the COVID / one-step-economy scenarios,
    be listed in an environment with dense logs, be captured in a
    hipGraph (rollout.GraphedStep) or restart inside the step (auto-reset): both would run steps and resets without its
    hooks, so on an environment with host components GraphedStep, the backend's whole-step calls (`step`,
    `step_sample_next`) and `set_auto_reset(True)` raise; step and reset it with env.step / env.reset.  Cost: one extra
    launch per stretch, the full-featured kernel instead of the configuration's instance, and whatever the hook's torch
    code costs -- an extension point, not the hot path.  tests/test_batched_component.py holds toy components against
    the same components added to the live reference."""
    comp_id = 0  # no device kernel
    is_batched_host_component = True

    def get_n_actions(self, agent_cls_name):
        return None

    def fill_config(self, cfg):
        return None

    def component_step(self, tensors):
        raise NotImplementedError

    def generate_observations(self, tensors):
        return {"a": {}, "p": {}}

    def additional_reset_steps(self, tensors, env_mask=None):
        """Called after the reset kernel; `env_mask`: the uint8 [n_envs] mask of the replicas that were reset (None:
        all).  Return True when state tensors were edited (the observations are then rewritten)."""
        return False


class ActingComponent(BatchedComponent):
    """A host component that ACTS: it owns action subspaces and their masks, the reference's component contract
    `get_n_actions` + `generate_masks` + `component_step` (F/base/base_component.py:159-176, 262-290).

    `get_n_actions(agent_cls_name)` ("BasicMobileAgent" / "BasicPlanner") returns None or 0 (no subspace), an int n (one
    subspace named "<Component>") or a list of (sub_name, n) (subspaces "<Component>.<sub_name>"; n == 0 entries are
    skipped, a "." in a sub-name is a NameError, any other type a TypeError: F/base/base_agent.py:116-153).  The subspaces
    take their place in the action layout -- single-action indices, multi-action columns, flattened mask entries,
    `flatten_masks=False` keys -- by the component's position in `components` relative to the built-in ones, exactly as
    the reference lays them out (F/base/base_agent.py:97-180).

        @foundation.components.add
        class Tithe(foundation.ActingComponent):
            name = "Tithe"
            required_entities = ["Coin"]
            agent_subclasses = ["BasicMobileAgent"]

            def get_n_actions(self, agent_cls_name):
                return 3 if agent_cls_name == "BasicMobileAgent" else None

            def component_step(self, t):
                k = self.agent_actions(t).to(t["inv_coin"].dtype)          # int32 [n_envs, n_agents]: 0 = NO-OP, 1..3
                k = k * (t["inv_coin"] >= k)                                # masks are advice: a forbidden choice does nothing
                t["inv_coin"] += k.sum(1, keepdim=True) / k.shape[1] - k

            def generate_masks(self, t, completions=0):
                ks = torch.arange(1, 4, device=t["inv_coin"].device)
                return {"a": t["inv_coin"][:, :, None] >= ks}               # [n_envs, n_agents, 3], any dtype

    Inside `component_step(tensors)`, `self.agent_actions(tensors, sub_name=None)` is the int32 [n_envs, n_agents] view
    and `self.planner_actions(tensors, sub_name=None)` the int32 [n_envs] view of what the actors chose in this step
    (0 = NO-OP, 1 .. n = the choice; the reference's `agent.get_component_action(...)`): zero-copy columns of the device
    tensors `host_actions_a` / `host_actions_p`, which the step's first launch decodes from the action buffers.  An index
    outside the action space raises the replica's error flag and reads as NO-OP, as for the built-in components.

    `generate_masks(tensors, completions=0)` returns {"a": M or {sub_name: M}, "p": M or {sub_name: M}} with M of shape
    [n_envs, n_agents, n] (agents) / [n_envs, n] (planner), any dtype (non-zero = allowed); a missing entry means all
    ones.  It is called on the end-of-step state (after the resource regeneration) and at reset after every reset hook,
    as the reference calls `_generate_masks` behind `scenario_step` (F/base/base_env.py:700-703); the environment writes
    the result into the arena's `obs_a_action_mask` / `obs_p_action_mask` tensors -- the ones the device samplers read --
    before env.step / env.reset return, every step (the step kernel may rewrite a mask row in between; it puts 1.0 into
    these entries).  `completions`: the int32 [n_envs] tensor of completed episodes.  As in the reference the masks are
    advice: nothing enforces them on incoming actions, the component decides what a forbidden choice does.

    Everything BatchedComponent documents as refused stays refused: COVID and one-step-economy scenarios, dense logs,
    rollout.GraphedStep, auto-reset and the backend's whole-step calls.  The device samplers need a multi-action
    planner's rows to be equally long: with a planner subspace of another size than the tax brackets' they raise
    NotImplementedError (sample the planner's actions on the host).  tests/test_acting_component.py holds toy components
    against the same components added to the live reference."""
    owns_action_subspaces = True

    def generate_masks(self, tensors, completions=0):
        return {}

    def _column(self, who, sub_name):
        cols = getattr(self, "_action_columns", None)
        if cols is None:
            raise RuntimeError("component {!r} is not part of an environment yet".format(self.name))
        if sub_name not in cols[who]:
            raise KeyError("component {!r} has no {} action subspace {!r} (it has: {})".format(
                self.name, "agent" if who == "a" else "planner", sub_name, sorted(cols[who], key=str)))
        return cols[who][sub_name]

    def agent_actions(self, tensors, sub_name=None):
        return tensors["host_actions_a"][:, :, self._column("a", sub_name)]

    def planner_actions(self, tensors, sub_name=None):
        return tensors["host_actions_p"][:, self._column("p", sub_name)]


component_registry = Registry(BaseComponent)
