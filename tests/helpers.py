"""Shared test helpers: golden fixtures, config building, state comparison."""
import glob
import contextlib
import json
import os

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")

INT_FIELDS = ["stone", "wood", "house_owner", "loc_r", "loc_c", "inv_res", "esc_res",
              "cda_n_bids", "cda_n_asks", "cda_n_orders", "cda_bid_hist", "cda_ask_hist",
              "tax_cycle_pos", "tax_last_completions", "tax_rate_idx", "timestep", "completions", "auto_warmup", "mt_pos",
              "labor_first_step", "saez_buffer_len", "saez_reached_min_samples"]
F64_FIELDS = ["inv_coin", "esc_coin", "labor", "build_payment", "build_skill",
              "bonus_gather_prob", "util", "cda_price_history", "tax_last_coin",
              "tax_last_income", "tax_last_marginal_rate", "tax_total_collected", "skill",
              "production", "saez_elas", "saez_running_avg_tax_rates", "tax_saez_bracket_rates"]


def golden_names():
    """Gather-trade-build / one-step-economy fixtures (the COVID ones have their own format)."""
    names = sorted(os.path.basename(p)[:-4] for p in glob.glob(os.path.join(GOLDEN, "*.npz")))
    return [n for n in names if not n.startswith("c4_covid") and not n.startswith("custom_")]


def custom_golden_names():
    """Fixtures with user-registered components (oracle/gen_golden_custom.py)."""
    return sorted(os.path.basename(p)[:-4] for p in glob.glob(os.path.join(GOLDEN, "custom_*.npz")))


def covid_golden_names():
    return sorted(os.path.basename(p)[:-4] for p in glob.glob(os.path.join(GOLDEN, "c4_covid*.npz")))


def load_covid_golden(name):
    with np.load(os.path.join(GOLDEN, name + ".npz")) as z:
        g = {k: z[k] for k in z.files}
    g["cfg"] = json.loads(str(g["config_json"]))
    g["cfg"]["components"] = [tuple(c) for c in g["cfg"]["components"]]
    return g


def load_golden(name):
    with np.load(os.path.join(GOLDEN, name + ".npz")) as z:
        g = {k: z[k] for k in z.files}
    g["cfg"] = json.loads(str(g["cfg_json"]))
    if "construction_seed" in g:
        # scenarios that draw from the GLOBAL NumPy stream in their constructor (SplitLayout's
        # ranked skills): make_env re-seeds the global stream the way the generator did
        g["cfg"]["_construction_seed"] = int(g["construction_seed"])
    if "s0_skill" in g:
        # SimpleLabor estimates its skills from the GLOBAL NumPy stream at construction
        # (simple_labor.py:66-74); the fixture carries the values the reference drew.
        for comp in g["cfg"]["components"]:
            if comp[0] == "SimpleLabor":
                comp[1]["skills"] = [float(x) for x in g["s0_skill"]]
    return g


def make_env(cfg, n_envs=1, **extra):
    """Host env (no device work happens until reset/step)."""
    from ai_economist_amd import foundation

    kw = dict(cfg)
    cseed = kw.pop("_construction_seed", None)
    if cseed is not None:
        np.random.seed(cseed)
    scenario = kw.pop("scenario_name")
    kw["components"] = [tuple(c) for c in kw["components"]]
    kw.update(extra)
    return foundation.make_env_instance(scenario, n_envs=n_envs, **kw)


@contextlib.contextmanager
def dev_library():
    """Environments whose device backend is created inside this block load libaie_hip_dev.so (the -DAIE_DEV build:
    aie_dev_* hooks, traced kernels); everything else in the process stays on the shipping library."""
    old = os.environ.get("AIE_DEV_LIB")
    os.environ["AIE_DEV_LIB"] = "1"
    try:
        yield
    finally:
        if old is None:
            del os.environ["AIE_DEV_LIB"]
        else:
            os.environ["AIE_DEV_LIB"] = old


def dev_switches():
    """The development switches by name ({"AIE_DEV_SKIP_REGEN": 2, ...}): tools/devlib.py reads them out of
    csrc/aie_layout.h."""
    import importlib.util

    spec = importlib.util.spec_from_file_location("devlib", os.path.join(ROOT, "tools", "devlib.py"))
    devlib = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(devlib)
    return devlib.switches()


def state_from_golden(g, prefix, t=None):
    out = {}
    for k, v in g.items():
        if k.startswith(prefix):
            out[k[len(prefix):]] = v if t is None else v[t]
    return out


def book_equal(n_a, book_a, n_b, book_b):
    """Order books: only the first n entries of each [R, M] row are meaningful."""
    for r in range(2):
        if int(n_a[r]) != int(n_b[r]):
            return False
        if not np.array_equal(book_a[r, : n_a[r]], book_b[r, : n_b[r]]):
            return False
    return True


def compare_state(got, want, where="", f64_tol=1e-9):
    """got/want: {field: array} for ONE replica.  Integer state bit-exact, f64 within tol."""
    for k in INT_FIELDS:
        if k in want and k in got:
            assert np.array_equal(np.asarray(got[k]), np.asarray(want[k])), (
                "%s: integer field %s differs\n got=%s\nwant=%s" % (where, k, got[k], want[k]))
    if "cda_bids" in want and "cda_bids" in got:
        assert book_equal(got["cda_n_bids"], got["cda_bids"], want["cda_n_bids"], want["cda_bids"]), (
            "%s: bid book differs" % where)
        assert book_equal(got["cda_n_asks"], got["cda_asks"], want["cda_n_asks"], want["cda_asks"]), (
            "%s: ask book differs" % where)
    if "saez_buffer_filled" in want and "saez_buffer" in got:  # the filled prefix of the sample buffer
        m = int(want["saez_buffer_len"])
        np.testing.assert_allclose(np.asarray(got["saez_buffer"])[:m], np.asarray(want["saez_buffer_filled"])[:m], rtol=f64_tol,
                                   atol=f64_tol, err_msg="%s: saez buffer" % where)
    for k in F64_FIELDS:
        if k in want and k in got:
            np.testing.assert_allclose(np.asarray(got[k]), np.asarray(want[k]), rtol=f64_tol,
                                       atol=f64_tol, err_msg="%s: f64 field %s" % (where, k))


def oracle_host_pre_reset(env, oracle, which=None):
    """What BaseEnvironment.host_pre_reset does on the device, on an OracleEnv: scenarios
    with a host-side reset part (uniform/...: a fresh layout from the replica's own MT19937
    stream) run it here before oracle.reset()."""
    if not hasattr(env, "generate_layout") or getattr(env, "layouts_on_device", False):
        return  # fixed layouts, or layouts drawn inside reset (device kernel / restatement alike)
    which = range(oracle.E) if which is None else which
    rs = np.random.RandomState()
    for e in which:
        rs.set_state(("MT19937", oracle.t["mt"][e].copy(), int(oracle.t["mt_pos"][e]),
                      int(oracle.t["mt_has_gauss"][e]), float(oracle.t["mt_gauss"][e])))
        oracle.t["cell_flags"][e] = env.generate_layout_flags(rs)
        st = rs.get_state()
        oracle.t["mt"][e] = st[1]
        oracle.t["mt_pos"][e] = st[2]
        oracle.t["mt_has_gauss"][e] = st[3]
        oracle.t["mt_gauss"][e] = st[4]


def random_gtb_config(seed):
    """A random but valid gather-trade-build configuration (deterministic in `seed`): scenario
    class, world / layout, number of agents, component subset, order and kwargs, action modes,
    observation and reward options.  Used to widen parity coverage beyond the hand-picked
    variants (reference-marked CPU test: oracle vs live reference; GPU test: HIP vs oracle)."""
    rng = np.random.RandomState(1000 + seed)
    pick = lambda xs: xs[rng.randint(len(xs))]  # noqa: E731
    layouts = {(25, 25): ["quadrant_25x25_20each_30clump.txt", "uniform_25x25_25each_65clump.txt",
                          "closed_quadrant_25x25_20each_30clump.txt", "env-pure_and_mixed-25x25.txt",
                          "quadrant_25x25_20each_30clump_no_water.txt"],
               (15, 15): ["env-pure_and_mixed-15x15.txt"], (14, 14): ["top_wood_bottom_stone_14x14.txt"],
               (40, 40): ["quadrant_40x40_50each.txt"]}
    kind = pick(["file", "file", "file", "uniform", "quadrant", "multi_zone"])
    # (isoelastic_eta == 1 is left out: it raises inside the reference itself, rewards.py:38)
    cfg = dict(episode_length=int(pick([30, 45, 70])), starting_agent_coin=float(pick([0, 5, 12.5])),
               multi_action_mode_agents=bool(rng.rand() < 0.35), multi_action_mode_planner=bool(rng.rand() < 0.7),
               allow_observation_scaling=bool(rng.rand() < 0.8), planner_gets_spatial_info=bool(rng.rand() < 0.7),
               full_observability=bool(rng.rand() < 0.2), mobile_agent_observation_range=int(pick([1, 3, 5, 7])),
               isoelastic_eta=float(pick([0.0, 0.23, 0.5, 0.9])), energy_cost=float(pick([0.0, 0.21, 0.5])),
               planner_reward_type=pick(["coin_eq_times_productivity", "inv_income_weighted_coin_endowments",
                                         "inv_income_weighted_utility"]),
               mixing_weight_gini_vs_coin=float(pick([0.0, 0.3, 1.0])))
    if rng.rand() < 0.4:
        cfg.update(energy_warmup_constant=float(pick([2, 50])), energy_warmup_method=pick(["decay", "auto"]))
    if kind == "file":
        hw = pick(list(layouts))
        cfg.update(scenario_name="layout_from_file/simple_wood_and_stone", world_size=list(hw),
                   env_layout_file=pick(layouts[hw]), resource_regen_prob=float(pick([0.01, 0.1, 0.5])))
    else:
        side = int(pick([12, 16, 20]))
        cfg.update(scenario_name=kind + "/simple_wood_and_stone", world_size=[side, side],
                   starting_wood_coverage=float(pick([0.05, 0.1])), starting_stone_coverage=float(pick([0.05, 0.1])),
                   wood_regen_weight=float(pick([0.01, 0.2])), stone_regen_weight=float(pick([0.01, 0.2])),
                   wood_max_health=int(pick([1, 2])), stone_max_health=int(pick([1, 3])))
        rng3 = np.random.RandomState(8000 + seed)  # own stream: keeps the draws of older seeds stable
        if rng3.rand() < 0.6:  # regeneration probability from the d x d neighbourhood of source blocks
            cfg.update(wood_regen_halfwidth=int(rng3.randint(0, 4)), stone_regen_halfwidth=int(rng3.randint(0, 4)))
            if cfg["wood_regen_halfwidth"]:
                cfg["wood_max_health"] = 1
            if cfg["stone_regen_halfwidth"]:
                cfg["stone_max_health"] = 1
            cfg.update(wood_regen_weight=float(rng3.choice([0.2, 0.9])), stone_regen_weight=float(rng3.choice([0.3, 1.0])))
        if kind == "multi_zone":
            cfg.update(num_partitions_row=4, num_partitions_col=4, num_wood_zones=3, num_stone_zones=3,
                       num_wood_and_stone_zones=2)
    small = min(cfg["world_size"]) <= 8
    cfg["n_agents"] = int(pick([2, 3]) if small else pick([2, 4, 5, 7, 10]))
    comps = []
    if rng.rand() < 0.85:
        comps.append(["Build", dict(payment=int(pick([5, 10])), skill_dist=pick(["none", "pareto", "lognormal"]),
                                    payment_max_skill_multiplier=int(pick([1, 3])), build_labor=float(pick([1.0, 10.0])))])
    if rng.rand() < 0.8:
        comps.append(["ContinuousDoubleAuction", dict(max_bid_ask=int(pick([5, 10, 16])), order_labor=float(pick([0.0, 0.25])),
                                                      order_duration=int(pick([3, 12, 50])), max_num_orders=int(pick([1, 3, 5])))])
    comps.append(["Gather", dict(move_labor=float(pick([0.5, 1.0])), collect_labor=float(pick([1.0, 2.0])),
                                 skill_dist=pick(["none", "pareto", "lognormal"]))])
    if rng.rand() < 0.8:
        tax = dict(period=int(pick([7, 10, 25])), disable_taxes=bool(rng.rand() < 0.15))
        model = pick(["model_wrapper", "model_wrapper", "us-federal-single-filer-2018-scaled", "fixed-bracket-rates"])
        tax["tax_model"] = model
        if model == "us-federal-single-filer-2018-scaled":
            tax["bracket_spacing"] = "us-federal"
        else:
            tax["bracket_spacing"] = pick(["us-federal", "linear", "log"])
            if tax["bracket_spacing"] != "us-federal":
                tax.update(n_brackets=int(pick([3, 5])), top_bracket_cutoff=float(pick([20, 60])))
        if model == "model_wrapper":
            tax["rate_disc"] = float(pick([0.05, 0.1, 0.25]))
        if model == "fixed-bracket-rates":
            nb = 7 if tax["bracket_spacing"] == "us-federal" else tax["n_brackets"]
            tax["fixed_bracket_rates"] = [round(float(x), 3) for x in np.sort(rng.rand(nb))]
        if rng.rand() < 0.3:
            tax["tax_annealing_schedule"] = [int(pick([-1, 0, 1])), float(pick([0.3, 0.6]))]
        comps.append(["PeriodicBracketTax", tax])
    rng.shuffle(comps)
    # passive equal-split component at a random position (own stream: keeps the draws above stable)
    rng2 = np.random.RandomState(7000 + seed)
    if rng2.rand() < 0.2:
        comps.insert(int(rng2.randint(len(comps) + 1)), ["WealthRedistribution", {}])
    cfg["components"] = comps
    return cfg


def random_ose_config(seed):
    """A random valid one-step-economy configuration (deterministic in `seed`)."""
    rng = np.random.RandomState(2000 + seed)
    pick = lambda xs: xs[rng.randint(len(xs))]  # noqa: E731
    n = int(pick([2, 5, 17, 33, 64, 100, 128]))
    tax = dict(period=int(pick([1, 1, 2])), disable_taxes=bool(rng.rand() < 0.1))
    model = pick(["model_wrapper", "model_wrapper", "us-federal-single-filer-2018-scaled", "fixed-bracket-rates"])
    tax["tax_model"] = model
    tax["bracket_spacing"] = "us-federal" if model != "fixed-bracket-rates" or rng.rand() < 0.5 else pick(["linear", "log"])
    if tax["bracket_spacing"] != "us-federal":
        tax.update(n_brackets=int(pick([3, 6])), top_bracket_cutoff=float(pick([50, 200])))
    if model == "model_wrapper":
        tax["rate_disc"] = float(pick([0.05, 0.1]))
        tax["usd_scaling"] = float(pick([1000.0, 500.0]))
    if model == "fixed-bracket-rates":
        nb = 7 if tax["bracket_spacing"] == "us-federal" else tax["n_brackets"]
        tax["fixed_bracket_rates"] = [round(float(x), 3) for x in np.sort(rng.rand(nb))]
    if rng.rand() < 0.25:
        tax["tax_annealing_schedule"] = [int(pick([-1, 0])), float(pick([0.2, 0.5]))]
    labor = dict(mask_first_step=bool(rng.rand() < 0.7), payment_max_skill_multiplier=int(pick([2, 3])),
                 pareto_param=float(pick([3.0, 4.0])))
    comps = [["SimpleLabor", labor], ["PeriodicBracketTax", tax]]
    if rng.rand() < 0.3:
        comps = comps[::-1]
    cfg = dict(scenario_name="one-step-economy", world_size=[1, 1], n_agents=n, episode_length=int(pick([1, 2, 5])),
               components=comps, multi_action_mode_planner=bool(rng.rand() < 0.7),
               allow_observation_scaling=bool(rng.rand() < 0.8),
               agent_reward_type=pick(["coin_minus_labor_cost", "isoelastic_coin_minus_labor"]),
               isoelastic_eta=float(pick([0.0, 0.23, 0.6])), labor_exponent=float(pick([1.5, 2.0, 3.5])),
               labor_cost=float(pick([0.5, 1.0])),
               planner_reward_type=pick(["coin_eq_times_productivity", "inv_income_weighted_utility"]),
               mixing_weight_gini_vs_coin=float(pick([0.0, 0.4])))
    return cfg


def random_covid_config(seed):
    """A random valid CovidAndEconomySimulation configuration (dates within the complete part
    of the real-world tables)."""
    rng = np.random.RandomState(3000 + seed)
    pick = lambda xs: xs[rng.randint(len(xs))]  # noqa: E731
    start = pick(["2020-02-25", "2020-03-22", "2020-05-01", "2020-08-15", "2020-11-01"])
    vac = {"2020-02-25": "2020-03-20", "2020-03-22": "2020-05-01", "2020-05-01": "2020-05-11",
           "2020-08-15": "2021-01-12", "2020-11-01": "2020-11-20"}[start]
    return dict(
        collate_agent_step_and_reset_data=True,
        components=[("ControlUSStateOpenCloseStatus", {"action_cooldown_period": int(pick([1, 7, 28]))}),
                    ("FederalGovernmentSubsidy", {"num_subsidy_levels": int(pick([5, 20])),
                                                  "subsidy_interval": int(pick([7, 30, 90])),
                                                  "max_annual_subsidy_per_person": float(pick([5000, 20000]))}),
                    ("VaccinationCampaign", {"daily_vaccines_per_million_people": int(pick([1000, 4500])),
                                             "delivery_interval": int(pick([1, 3, 7])),
                                             "vaccine_delivery_start_date": vac})],
        economic_reward_crra_eta=float(pick([0.5, 2, 3.5])), episode_length=int(pick([40, 75])),
        flatten_masks=True, flatten_observations=False,
        health_priority_scaling_agents=float(pick([0.3, 1, 2.5])), health_priority_scaling_planner=float(pick([0.45, 1])),
        infection_too_sick_to_work_rate=float(pick([0.05, 0.1, 0.3])), multi_action_mode_agents=False,
        multi_action_mode_planner=False, n_agents=51, path_to_data_and_fitted_params="",
        pop_between_age_18_65=float(pick([0.5, 0.6])), risk_free_interest_rate=float(pick([0.0, 0.03, 0.1])),
        reward_normalization_factor=float(pick([1, 4])), world_size=[1, 1], start_date=start,
        use_real_world_data=False, use_real_world_policies=False)


GTB = [["Build", {}], ["ContinuousDoubleAuction", {"max_num_orders": 5}], ["Gather", {}], ["PeriodicBracketTax", {}]]
C2 = dict(scenario_name="layout_from_file/simple_wood_and_stone", n_agents=4, world_size=[25, 25],
          episode_length=1000, components=GTB, starting_agent_coin=10,
          env_layout_file="quadrant_25x25_20each_30clump.txt")
C1_INSTANCE = dict(scenario_name="uniform/simple_wood_and_stone", n_agents=4, world_size=[15, 15], episode_length=1000,
                   components=[["Build", {}], ["Gather", {}]], starting_agent_coin=10, starting_stone_coverage=0.10,
                   starting_wood_coverage=0.10)


# ---- shapes where a step kernel typically breaks: non-square worlds, the 4096-cell limit of device-drawn layouts, order
# books on either side of 64 slots, gini's branches.  The same configurations are pinned against the live reference
# (tests/test_oracle_vs_reference_shapes.py) and run on the device against the oracle (tests/test_gpu_shapes.py). ----
def _shape_cfg(kind, h, w, **kw):
    cfg = dict(scenario_name=kind + "/simple_wood_and_stone", n_agents=4, world_size=[h, w], episode_length=20,
               components=[["Build", {}], ["ContinuousDoubleAuction", {"max_num_orders": 4, "order_duration": 15}],
                           ["Gather", {}], ["PeriodicBracketTax", {"period": 7}]],
               starting_agent_coin=5, starting_wood_coverage=0.06, starting_stone_coverage=0.06,
               wood_regen_weight=0.3, stone_regen_weight=0.3)
    cfg.update(kw)
    return cfg


SHAPE_CASES = {
    # d x d window counts of source blocks (regen_halfwidth > 0, max_health 1); observation windows wider than the short
    # side only
    "uniform_12x37_source_counts": _shape_cfg("uniform", 12, 37, wood_regen_halfwidth=2, stone_regen_halfwidth=1,
                                              mobile_agent_observation_range=7),
    "uniform_37x12_source_counts": _shape_cfg("uniform", 37, 12, wood_regen_halfwidth=2, stone_regen_halfwidth=2,
                                              mobile_agent_observation_range=7, planner_gets_spatial_info=False),
    # max_health > 1 beside a window: the general convolution (regen_general) of max(map, source) per step
    "uniform_12x37_general_regen": _shape_cfg("uniform", 12, 37, wood_regen_halfwidth=2, stone_max_health=3,
                                              stone_regen_halfwidth=1, mobile_agent_observation_range=3),
    "uniform_37x12_general_regen": _shape_cfg("uniform", 37, 12, wood_max_health=2, wood_regen_halfwidth=3,
                                              stone_regen_halfwidth=0),
    # 3840 cells: device-drawn layouts with rows wider than a wavefront, > 128 source blocks (row-by-row regeneration)
    "uniform_24x160": _shape_cfg("uniform", 24, 160, starting_wood_coverage=0.05, starting_stone_coverage=0.05,
                                 mobile_agent_observation_range=15),
    "uniform_160x24": _shape_cfg("uniform", 160, 24, starting_wood_coverage=0.05, starting_stone_coverage=0.05,
                                 mobile_agent_observation_range=12, planner_gets_spatial_info=False),
    "quadrant_20x30": _shape_cfg("quadrant", 20, 30, starting_wood_coverage=0.1, starting_stone_coverage=0.1),
    "quadrant_30x20": _shape_cfg("quadrant", 30, 20, starting_wood_coverage=0.1, starting_stone_coverage=0.1,
                                 wood_regen_halfwidth=1, stone_regen_halfwidth=2, mobile_agent_observation_range=11),
    "multi_zone_15x28": _shape_cfg("multi_zone", 15, 28, num_partitions_row=3, num_partitions_col=4, num_wood_zones=3,
                                   num_stone_zones=3, num_wood_and_stone_zones=2, starting_wood_coverage=0.08,
                                   starting_stone_coverage=0.08),
    # the device layout path's 4096-cell limit from both sides (64 x 65 is drawn on the host)
    "uniform_65x63": _shape_cfg("uniform", 65, 63, n_agents=3, starting_wood_coverage=0.02, starting_stone_coverage=0.02,
                                components=[["Build", {}], ["Gather", {}]]),
    "uniform_64x64": _shape_cfg("uniform", 64, 64, n_agents=3, starting_wood_coverage=0.02, starting_stone_coverage=0.02,
                                components=[["Build", {}], ["Gather", {}]], wood_regen_halfwidth=1),
    "uniform_64x65": _shape_cfg("uniform", 64, 65, n_agents=3, starting_wood_coverage=0.02, starting_stone_coverage=0.02,
                                components=[["Build", {}], ["Gather", {}]]),
    # the whole map as the agents' observation, with and without the planner's spatial view
    "full_observability_18x11": _shape_cfg("uniform", 18, 11, full_observability=True),
    "full_observability_11x18_planner_blind": _shape_cfg("quadrant", 11, 18, full_observability=True,
                                                         planner_gets_spatial_info=False),
}

# quadrant/ puts a water row at width // 2 and a water column at height // 2 (the reference's own swap): shapes with
# width // 2 >= height or height // 2 >= width raise IndexError in the reference's constructor, and in the product's
REFUSED_SHAPES = {"quadrant_9x30": _shape_cfg("quadrant", 9, 30), "quadrant_30x9": _shape_cfg("quadrant", 30, 9)}


def _agents_cfg(n, orders, **kw):
    cfg = dict(scenario_name="layout_from_file/simple_wood_and_stone", n_agents=n, world_size=[40, 40], episode_length=18,
               starting_agent_coin=60, resource_regen_prob=0.08, env_layout_file="quadrant_40x40_50each.txt",
               components=[["Build", {}], ["ContinuousDoubleAuction", {"max_num_orders": orders, "order_duration": 15}],
                           ["Gather", {}], ["PeriodicBracketTax", {"period": 6}]])
    cfg.update(kw)
    return cfg


# name -> configuration with all four components on the 40 x 40 quadrant file; the order book holds
# M = n_agents * max_num_orders slots: M <= 64 steps in a register-resident or LDS book of the non-log kernels, M > 64 on
# aie_step_kernel_log
AGENT_CASES = {
    "n16_book64": _agents_cfg(16, 4),
    "n21_book63": _agents_cfg(21, 3),
    "n32_book64": _agents_cfg(32, 2),
    "n61_book61": _agents_cfg(61, 1),
    "n62_book62": _agents_cfg(62, 1),
    "n13_book65": _agents_cfg(13, 5),
    "n33_book66": _agents_cfg(33, 2),
    # gini: pairwise sums below 30 agents, the sorted cumulative sum from 30 on
    "n29_coin_eq": _agents_cfg(29, 2, planner_reward_type="coin_eq_times_productivity", mixing_weight_gini_vs_coin=0.3),
    "n30_coin_eq": _agents_cfg(30, 2, planner_reward_type="coin_eq_times_productivity"),
    "n31_coin_eq": _agents_cfg(31, 2, planner_reward_type="coin_eq_times_productivity", mixing_weight_gini_vs_coin=0.6),
    "n30_inv_income_coin": _agents_cfg(30, 2, planner_reward_type="inv_income_weighted_coin_endowments",
                                       mixing_weight_gini_vs_coin=0.3),
    "n31_inv_income_utility": _agents_cfg(31, 2, planner_reward_type="inv_income_weighted_utility"),
}


def book_slots(cfg):
    """M = n_agents * max_num_orders: the order book's slots per side (0 without an auction)."""
    for name, kw in cfg["components"]:
        if name == "ContinuousDoubleAuction":  # (max_num_orders defaults to order_duration, 50)
            return cfg["n_agents"] * int(kw.get("max_num_orders") or kw.get("order_duration", 50))
    return 0


def _components_with(base, **per_component):
    return [[name, dict(kw, **per_component.get(name, {}))] for name, kw in base]


def _phase_yaml(k):
    from ai_economist_amd import _specs

    kw = dict(_specs.PHASE1 if k == 1 else _specs.PHASE2)
    kw["components"] = [[name, dict(c)] for name, c in kw["components"]]
    return dict(kw, scenario_name="layout_from_file/simple_wood_and_stone")


# An instance stands for a FAMILY (aie_layout.h: aie_spec_normalize): the configuration's scalars and value tables
# are read from the run-time block.  name -> (configuration, expected to run on a compile-time instance)
FAMILY_CASES = {
    "c2": (dict(C2), True),
    "c3": (dict(C2, n_agents=10), True),
    "c1": (dict(C1_INSTANCE), True),
    # VERDICT r3 #2's own example
    "c2_coin15_eta05_len500": (dict(C2, starting_agent_coin=15, isoelastic_eta=0.5, episode_length=500), True),
    # every scalar at once, episode ends inside the run (the reset instance reads starting coin, Build payment, ...)
    "c2_every_scalar": (dict(C2, episode_length=70, starting_agent_coin=3.5, isoelastic_eta=0.4, energy_cost=0.35,
                             resource_regen_prob=0.04, mixing_weight_gini_vs_coin=0.3,
                             components=_components_with(
                                 GTB, Build=dict(payment=15, payment_max_skill_multiplier=2, build_labor=7.0),
                                 ContinuousDoubleAuction=dict(order_duration=9, order_labor=0.5),
                                 Gather=dict(move_labor=2.0, collect_labor=3.0),
                                 PeriodicBracketTax=dict(period=20, usd_scaling=400.0))), True),
    "c2_rate_max": (dict(C2, components=_components_with(GTB, PeriodicBracketTax=dict(rate_max=0.8))), False),  # 17 rates, not 21
    "c3_short_taxes": (dict(C2, n_agents=10, episode_length=55, starting_agent_coin=0, energy_cost=0.1,
                            components=_components_with(GTB, PeriodicBracketTax=dict(period=7),
                                                        ContinuousDoubleAuction=dict(order_duration=3))), True),
    "c1_other_coverage": (dict(C1_INSTANCE, episode_length=45, starting_stone_coverage=0.2, starting_wood_coverage=0.05,
                               starting_agent_coin=1, isoelastic_eta=0.1,
                               components=[["Build", {"payment": 4, "build_labor": 3.0}], ["Gather", {"move_labor": 0.5}]]),
                          True),
    # the reference's training YAMLs (tutorials/rllib/phase1|phase2/config.yaml), dense_log_frequency included: the
    # logged replica takes the full-featured kernel while an episode is logged, everything else the instance
    "phase2_yaml": (dict(_phase_yaml(2), dense_log_frequency=20), True),
    "phase1_yaml": (dict(_phase_yaml(1), dense_log_frequency=20), True),
    "phase2_yaml_other_scalars": (dict(_phase_yaml(2), episode_length=60, energy_cost=0.3, isoelastic_eta=0.5), True),
    # scalars whose VALUE shapes the code stay out of the family: log utility, the energy warm-up
    "c2_eta_one": (dict(C2, isoelastic_eta=1.0), False),
    "c2_energy_warmup": (dict(C2, energy_warmup_constant=500), False),
    # and so does anything structural
    "c2_six_orders": (dict(C2, components=_components_with(GTB, ContinuousDoubleAuction=dict(max_num_orders=6))), False),
}


# ---- the policy sampler (csrc/aie_trainer_math.h: aie_sampler_exp, aie_sampler_entry_rng, the scan's order), transcribed in
# plain Python: IEEE double multiplies and adds in the header's order, nothing else ----
def _f32_nearest(fr):
    """The float32 nearest to the exact rational `fr`, ties to even (one rounding, as a hardware fma rounds)."""
    from fractions import Fraction

    f = np.float32(float(fr))  # within one unit of the answer (float(fr) is itself correctly rounded to float64)
    best = None
    for c in (np.nextafter(f, np.float32(-np.inf)), f, np.nextafter(f, np.float32(np.inf))):
        if not np.isfinite(c):
            continue
        key = (abs(Fraction(float(c)) - fr), int(np.float32(c).view(np.uint32)) & 1)
        if best is None or key < best[0]:
            best = (key, np.float32(c))
    return best[1]


def fmaf(a, b, c):
    """a * b + c in float32 with ONE rounding (C's fmaf / v_fma_f32), through exact rational arithmetic."""
    from fractions import Fraction

    return _f32_nearest(Fraction(float(a)) * Fraction(float(b)) + Fraction(float(c)))


def sampler_expf(y):
    f32 = np.float32
    y = f32(y)
    if not (y > f32(-80.0)):
        return f32(0.0)
    n = np.rint(y * f32(float.fromhex("0x1.715476p+0")))  # float32 product, round half to even
    r = fmaf(n, f32(-float.fromhex("0x1.62e4p-1")), y)
    r = fmaf(n, f32(-float.fromhex("0x1.7f7d1cp-20")), r)
    p = f32(float.fromhex("0x1.6c16c2p-10"))
    for c in ("0x1.111112p-7", "0x1.555556p-5", "0x1.555556p-3", "0x1p-1", "0x1p+0", "0x1p+0"):
        p = fmaf(p, r, f32(float.fromhex(c)))
    return f32(np.ldexp(p, int(n)))


def sampler_uniform(rnd):
    return np.float32(rnd >> 9) * np.float32(2.0 ** -23) + np.float32(2.0 ** -24)


def sampler_entry_rng(slot_word, k):
    h = (slot_word + k * 0x9E3779B1) & 0xffffffff
    h ^= h >> 16
    h = (h * 0x7feb352d) & 0xffffffff
    h ^= h >> 15
    h = (h * 0x846ca68b) & 0xffffffff
    return h ^ (h >> 16)


def counter_rng(seed, env_id, t, slot):
    M64 = (1 << 64) - 1
    z = (seed + 0x9E3779B97F4A7C15 * (env_id + 1)) & M64
    z ^= ((t + 1) * 0xBF58476D1CE4E5B9) & M64
    z ^= ((slot + 1) * 0x94D049BB133111EB) & M64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M64
    z ^= z >> 31
    return z >> 32


def sampler_pick_row(logits, mask, rnd):
    """One action slot: float32 logits, mask (> 0.5 = allowed), the slot's 32-bit word -> the entry
    aie_sample_policy_actions picks (float32 arithmetic, operation for operation)."""
    f32 = np.float32
    n = len(logits)
    lg = [f32(v) for v in logits]
    ok = [bool(mask[k] > 0.5) and bool(lg[k] == lg[k]) for k in range(n)]
    if not any(ok):
        return 0
    M = max(lg[k] for k in range(n) if ok[k])
    u = sampler_uniform(rnd)
    nch = (n + 63) // 64
    seg = 64 if nch > 1 else (16 if n <= 16 else 32 if n <= 32 else 64)  # aie_sampler_segment
    zero = f32(0.0)
    T, choice, last_ok = zero, -1, -1
    for pas in ((0, 1) if nch > 1 else (1,)):
        carry = zero
        for ch in range(nch):
            v = [sampler_expf(lg[64 * ch + r] - M) if 64 * ch + r < n and ok[64 * ch + r] else zero for r in range(64)]
            for d in (1, 2, 4, 8):
                v = [v[r] + (v[r - d] if (r & 15) >= d else zero) for r in range(64)]
            if seg >= 32:
                v = [v[r] + v[(r & ~15) - 1] if (r >> 4) & 1 else v[r] for r in range(64)]
            if seg >= 64:
                v = [v[r] + v[31] if r >= 32 else v[r] for r in range(64)]
            tot = carry + v[seg - 1]
            if pas == 0:
                carry = tot
                continue
            if nch == 1:
                T = tot
            for r in range(64):
                k = 64 * ch + r
                if k < n and ok[k]:
                    last_ok = k
                    if choice < 0 and carry + v[r] > u * T:
                        choice = k
            carry = tot
        if pas == 0:
            T = carry
    return last_ok if choice < 0 else choice
