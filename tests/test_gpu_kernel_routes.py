"""Which kernel a call launches (csrc/aie_capi.hip: aie_select_step / aie_select_reset; the table in DESIGN.md section 3),
one case per row.  The development hook aie_dev_step_route names what the next aie_step and aie_reset of an environment
would launch, in the selectors' own words: "<step launches joined by ' + '> | <reset kernel>", a launch over a replica
range as name[lo,hi)xgrid.  Every case is an environment of 8 (or 5) replicas and a string comparison."""
import ctypes

import pytest

import bench
from helpers import AGENT_CASES, C1_INSTANCE, C2, dev_library, dev_switches, load_covid_golden, covid_golden_names, make_env
from test_acting_component import _registry_as_found, load_acting, register_toys  # noqa: F401  (the fixture applies here too)

pytestmark = pytest.mark.gpu
GENERIC = 1  # AIE_KERNEL_GENERIC


def _env(cfg, n_envs=8, make=make_env, **extra):
    with dev_library():
        env = make(cfg, n_envs=n_envs, device="cuda:0", **extra)
        env.backend
    return env


def _route(be):
    buf = ctypes.create_string_buffer(512)
    assert be.lib.aie_dev_step_route(be.handle, buf, len(buf)) == 0
    step, reset = buf.value.decode().split(" | ")
    return step, reset


def _instance(be):
    return be.lib.aie_step_kernel_instance(be.handle)


def _generic_by_lds(be):
    """Row 8: the six-wave twin when the LDS footprint keeps a CU at 12 workgroups or fewer anyway."""
    lds = (ctypes.c_int64 * 6)()
    assert be.lib.aie_dev_lds_bytes(be.handle, lds) == 0
    return "aie_step_kernel_r6" if lds[5] <= 12 else "aie_step_kernel"


def test_compile_time_instance_and_its_reset():
    be = _env(bench.C2_CFG).backend
    k = _instance(be)
    assert k >= 0
    assert _route(be) == ("aie_step_kernel_spec<%d>" % k, "aie_reset_kernel_spec<%d>" % k)


@pytest.mark.parametrize("cfg", [C2, AGENT_CASES["n16_book64"]], ids=["c2", "n16_book64"])
def test_generic_kernel_by_lds_footprint_and_the_plain_reset(cfg):
    be = _env(cfg).backend
    assert be.lib.aie_select_step_kernel(be.handle, GENERIC) == 0
    assert _route(be) == (_generic_by_lds(be), "aie_reset_kernel")


def test_generated_layouts_reset_with_the_layout_kernel():
    be = _env(C1_INSTANCE).backend
    k = _instance(be)
    assert k >= 0 and _route(be)[1] == "aie_reset_kernel_spec<%d>" % k
    assert be.lib.aie_select_step_kernel(be.handle, GENERIC) == 0
    assert _route(be) == (_generic_by_lds(be), "aie_reset_kernel_layout")


def test_skip_mask_on_an_instance_takes_the_traced_twin():
    be = _env(bench.C2_CFG).backend
    k = _instance(be)
    assert be.lib.aie_dev_set_skip_mask(be.handle, dev_switches()["AIE_DEV_SKIP_REWARDS"]) == 0
    assert _route(be) == ("aie_step_kernel_spec_trace<%d>" % k, "aie_reset_kernel")  # (the instances' resets have no hooks)
    assert be.lib.aie_dev_set_skip_mask(be.handle, 0) == 0
    assert _route(be) == ("aie_step_kernel_spec<%d>" % k, "aie_reset_kernel_spec<%d>" % k)
    assert be.lib.aie_select_step_kernel(be.handle, GENERIC) == 0  # no instance: switched-off phases need the full-featured kernel
    assert be.lib.aie_dev_set_skip_mask(be.handle, dev_switches()["AIE_DEV_SKIP_REWARDS"]) == 0
    assert _route(be)[0] == "aie_step_kernel_log"


def test_draw_window_takes_the_full_featured_kernel_and_survives_a_skip_mask_call():
    be = _env(bench.C2_CFG).backend
    k = _instance(be)
    assert be.lib.aie_dev_set_draw_window(be.handle, 40) == 0
    assert _route(be) == ("aie_step_kernel_log", "aie_reset_kernel")
    assert be.lib.aie_dev_set_skip_mask(be.handle, 0) == 0  # (a flag of the environment, not a bit of the mask)
    assert _route(be) == ("aie_step_kernel_log", "aie_reset_kernel")
    assert be.lib.aie_dev_set_draw_window(be.handle, 0) == 0
    assert _route(be) == ("aie_step_kernel_spec<%d>" % k, "aie_reset_kernel_spec<%d>" % k)


def test_saez_runs_its_formula_kernel_ahead_of_the_full_featured_kernel():
    from test_oracle_vs_reference import _saez_cfg

    be = _env(_saez_cfg("inverse_income")[0]).backend
    assert _route(be)[0] == "aie_saez_kernel + aie_step_kernel_log"


def test_host_action_subspace_takes_the_full_featured_kernel():
    register_toys()
    be = _env(load_acting("acting_tithe_mid_4ag")["cfg"]).backend
    assert _route(be)[0] == "aie_step_kernel_log"


def test_order_books_beyond_a_wavefront_take_the_full_featured_kernel():
    be = _env(AGENT_CASES["n13_book65"]).backend
    assert _route(be)[0] == "aie_step_kernel_log"


@pytest.mark.parametrize("E", [8, 5])
def test_dense_log_replica_splits_the_step_while_it_records(E):
    """One logged replica: workgroup 0 alone when E is a multiple of 8 (8 (L - 1) + 1 = 1), L = 1 workgroups otherwise."""
    be = _env(dict(C2, dense_log_frequency=20), n_envs=E).backend
    k = _instance(be)
    assert k >= 0
    be.set_dense_log_active(True)
    assert _route(be)[0] == "aie_step_kernel_log[0,1)x1 + aie_step_kernel_spec<%d>[1,%d)" % (k, E)
    be.set_dense_log_active(False)
    assert _route(be)[0] == "aie_step_kernel_spec<%d>" % k


def test_one_step_economy_instance_and_generic():
    be = _env(bench._c5_cfg()).backend
    k = _instance(be)
    assert k >= 0
    assert _route(be) == ("aie_ose_step_kernel_spec<%d>" % k, "aie_ose_reset_kernel")
    assert be.lib.aie_select_step_kernel(be.handle, GENERIC) == 0
    assert _route(be) == ("aie_ose_step_kernel", "aie_ose_reset_kernel")


@pytest.mark.parametrize("recurrence", [False, True], ids=["window-sums", "recurrence"])
def test_covid_by_filter_count_and_recurrence(recurrence):
    from test_covid_golden import hip_env

    cfg = load_covid_golden(covid_golden_names()[0])["cfg"]
    be = _env(cfg, make=hip_env, filter_recurrence=recurrence).backend
    F = int(be.cfg.covid.num_filters)
    step = "aie_covid_step_kernel<%d, %s>" % (F, "true" if recurrence else "false")
    if not recurrence:  # (the reference's taps are float32 values)
        step += " + aie_covid_window_kernel<%d, float>" % F
    assert _route(be) == (step, "aie_covid_reset_kernel")


def test_runtime_specialisation_runs_the_loaded_module():
    from test_gpu_parity import JIT_CASES

    env = _env(JIT_CASES["phase2_planner_blind"])
    be = env.backend
    assert _instance(be) == -1, "the case must not have a compile-time instance"
    if not env.specialize():
        pytest.skip("no run-time specialisation here: %s" % be.lib.aie_last_error(be.handle).decode())
    assert _instance(be) == 1000
    assert _route(be) == ("aie_jit_step", "aie_jit_reset")
    assert be.lib.aie_dev_set_skip_mask(be.handle, dev_switches()["AIE_DEV_SKIP_REWARDS"]) == 0
    assert _route(be) == ("aie_step_kernel_log", "aie_reset_kernel")  # (it has no traced twin)
