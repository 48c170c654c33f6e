"""The row-edge cases of tests/row_edges.py, CPU side: what keeps tests/test_gpu_policy_row_edges.py honest.

  * every case builds, and mask_keys gives exactly the lengths the table records;
  * aie_sampler_args_of (csrc/aie_trainer_math.h, compiled here with the host C compiler) gives the recorded log2 of the lanes
    per row for either class, and the condition aie_capi.hip's aie_policy_sampler branches on gives the recorded fast-or-
    generic choice -- so the device tests launch the instance they name; the evaluator's and the PPO loss's plans
    (csrc/aie_trainer_plan.h) take the recorded fast or generic path per class; the nine fast instances are all there;
  * oracle/'s sample_policy_actions equals the Python transcription (helpers.sampler_pick_row on counter_rng /
    sampler_entry_rng) in every slot, over steps that cross a tax day;
  * the restatement's row sampler draws from the masked softmax at 16, 17, 32, 33, 64, 65, 128 and 129 entries with the
    largest logit on the last entry (chi-square, the rule of test_sampler_draws_from_the_masked_softmax).
"""
import ctypes as C
import math
import os
import subprocess
import tempfile

import numpy as np
import pytest

import row_edges
from helpers import ROOT, counter_rng, make_env, sampler_entry_rng, sampler_pick_row

CSRC = os.path.join(ROOT, "ai-economist_amd", "csrc")

SHIM = r"""
#include <stdlib.h>
#include "aie_layout_build.h"
#include "aie_trainer_plan.h"
/* out: agents' (len, lsh, rows), planner's (len, lsh, rows), ragged, the generic sampler?, the evaluator's generic flags (a, p),
 * the PPO loss's generic flags (a, p) */
int shim_row_shapes(const aie_config* c, int* out, char* err, int n) {
  aie_params* p = (aie_params*)malloc(sizeof(aie_params));
  int rc = aie_build_params(c, p, NULL, err, (size_t)n);
  if (rc == AIE_OK) rc = aie_sampler_check(p, err, (size_t)n);
  if (rc == AIE_OK) {
    const aie_sampler_args S = aie_sampler_args_of(p, NULL);
    out[0] = S.agents.len, out[1] = S.agents.lsh, out[2] = S.agents.rows;
    out[3] = S.planner.len, out[4] = S.planner.lsh, out[5] = S.planner.rows;
    out[6] = S.ragged;
    out[7] = S.ragged || S.agents.len > 64 || S.planner.len > 64; /* aie_capi.hip: aie_policy_sampler */
    const float* fake = (const float*)(uintptr_t)0x7f0000000000ull; /* a plan dereferences nothing */
    aie_policy_eval_args E;
    rc = aie_plan_eval_rows(p, NULL, NULL, "shim", 3, fake, fake, fake, fake, err, (size_t)n, &E);
    out[8] = E.agents.generic, out[9] = E.planner.generic;
    aie_ppo_class k;
    memset(&k, 0, sizeof(k));
    k.logits = fake, k.masks = fake, k.actions = (const int32_t*)fake, k.logp_old = fake, k.adv = fake;
    k.grad_logits = (float*)fake, k.stats = (float*)fake, k.clip = 0.2f;
    aie_ppo_plan q;
    if (rc == AIE_OK) rc = aie_plan_ppo_loss(p, NULL, NULL, 3, &k, &k, NULL, (void*)fake, err, (size_t)n, &q);
    out[10] = q.A.agents.generic, out[11] = q.A.planner.generic;
  }
  free(p);
  return rc;
}
"""


@pytest.fixture(scope="module")
def shim():
    with tempfile.TemporaryDirectory() as d:
        src, so = os.path.join(d, "shim_rows.c"), os.path.join(d, "shim_rows.so")
        with open(src, "w") as f:
            f.write(SHIM)
        subprocess.run(["gcc", "-O1", "-ffp-contract=off", "-shared", "-fPIC", "-I" + CSRC, "-I" + os.path.join(ROOT, "include"), src,
                        "-o", so, "-lm"], check=True)
        lib = C.CDLL(so)
        lib.shim_row_shapes.argtypes = [C.c_void_p, C.POINTER(C.c_int), C.c_char_p, C.c_int]
        yield lib


@pytest.mark.parametrize("name", row_edges.CASES)
def test_case_builds_with_the_recorded_rows_and_instance(shim, name):
    from ai_economist_amd.foundation.obs_keys import mask_keys

    case = row_edges.case(name)
    env = make_env(case.cfg, n_envs=3)
    tab = mask_keys(env)
    assert not env.multi_action_mode_agents and bool(env.multi_action_mode_planner) == case.multi_p
    assert tab["sizes"]["a"] == case.len_a, (name, tab["sizes"])
    if case.multi_p:
        assert [size + 1 for _, _, size in tab["p"]] == [case.len_p] * case.rows_p, (name, tab["p"])
        assert tab["sizes"]["p"] == case.rows_p * case.len_p
    else:
        assert case.rows_p == 1 and tab["sizes"]["p"] == case.len_p, (name, tab["sizes"])
    cfg = env.build_config()
    out, err = (C.c_int * 12)(), C.create_string_buffer(512)
    assert shim.shim_row_shapes(C.addressof(cfg), out, err, 512) == 0, err.value
    assert (out[0], out[2], out[3], out[5], out[6]) == (case.len_a, case.n, case.len_p, case.rows_p, 0)
    assert (out[1], out[4]) == case.lsh, "%s: lanes per row 2^%d / 2^%d, the table says 2^%d / 2^%d" % ((name, out[1], out[4]) + case.lsh)
    assert bool(out[7]) == case.generic, name
    assert (bool(out[8]), bool(out[9])) == (case.len_a > 64, case.len_p > 64)
    assert (bool(out[10]), bool(out[11])) == case.ppo_generic
    # the edge the case is there for: a full segment, one entry over a segment size, or a last chunk of one entry
    edges = [ln for ln in (case.len_a, case.len_p) if ln in row_edges.SEGMENTS or ln - 1 in row_edges.SEGMENTS or ln % 64 == 1]
    assert edges or name == "a62_p64", name
    if case.n == 5:  # the agents' last work item holds fewer rows than fit a wave
        assert case.n % (64 >> case.lsh[0])


def test_the_table_reaches_every_fast_instance_and_the_generic_kernel():
    assert row_edges.FAST_INSTANCES == [(a, q) for a in (4, 5, 6) for q in (4, 5, 6) if (a, q) not in ((4, 4), (4, 6), (6, 5))]
    # (4,4), (4,6) and (6,5) are the workloads' own: rows of 6 + 12, 6 + 52 and 50 + 22 (test_policy_sampler_equals_its_cpu_restatement);
    # the new ones are the five that no test launched
    assert {(4, 5), (5, 5), (5, 6), (6, 4), (6, 6)} <= set(row_edges.FAST_INSTANCES)
    generic = [row_edges.case(c) for c in row_edges.CASES if row_edges.case(c).generic]
    assert any(c.len_a % 64 == 1 and c.len_p % 64 == 1 for c in generic) and any(c.len_p == 129 for c in generic)


@pytest.mark.parametrize("name", row_edges.CASES)
def test_oracle_sampler_equals_the_transcription(name):
    """12 steps of 2 replicas (the planner's masks open on the tax days, steps 0 and 10), N(0, 3^2) logits."""
    from oracle_lib import OracleEnv

    case = row_edges.case(name)
    E, seed, off = 2, 41, 500
    env = make_env(case.cfg, n_envs=E)
    o = OracleEnv(env.build_config(), env.layout_planes())
    o.seed(5)
    o.reset()
    rows = case.rows()
    MA, MP = o.t["obs_a_action_mask"].shape[-1], o.t["obs_p_action_mask"].shape[-1]
    assert (MA, MP) == (case.len_a, case.rows_p * case.len_p)
    per_env = case.n + case.rows_p
    rs = np.random.RandomState(len(name))
    opened, picks_p = 0, set()
    for t in range(12):
        la = (rs.randn(E, case.n, MA) * 3).astype(np.float32)
        lp = (rs.randn(E, MP) * 3).astype(np.float32)
        ma, mp = o.t["obs_a_action_mask"].copy(), o.t["obs_p_action_mask"].copy()
        a, p = o.sample_policy_actions(la, lp, seed, off, width_a=1, width_p=case.rows_p)
        assert int(o.t["sample_t"][0]) == t + 1
        for e in range(E):
            base = counter_rng(seed, off + e, t, per_env)
            for i in range(case.n):
                assert a[e, i, 0] == sampler_pick_row(la[e, i], ma[e, i], sampler_entry_rng(base, i)), (name, t, e, i)
            for s, (lo, ln) in enumerate(rows["p"]):
                want = sampler_pick_row(lp[e, lo:lo + ln], mp[e, lo:lo + ln], sampler_entry_rng(base, case.n + s))
                assert p[e, s] == want, (name, t, e, s)
        opened += int((mp[:, 1:] > 0.5).any())
        picks_p.update(p.reshape(-1).tolist())
        o.step(a.reshape(E, -1), p)
    assert opened >= 2 and len(picks_p) > 1, "the planner's rows never opened"


@pytest.mark.parametrize("n", [16, 17, 32, 33, 64, 65, 128, 129])
def test_row_sampler_draws_from_the_masked_softmax_at_the_edges(n):
    from oracle_lib import lib

    L = lib()
    N = 20000
    rs = np.random.RandomState(100 + n)
    lg, mask = row_edges.edge_logits(n, rs)
    allowed = mask > 0.5
    assert allowed[n - 1] and lg[n - 1] == lg.max() and (~allowed).sum() == (n - 1) // 4
    counts = np.zeros(n)
    pl, pm = lg.ctypes.data_as(C.c_void_p), mask.ctypes.data_as(C.c_void_p)
    for t in range(N):  # the product's words: one per (replica, draw index), hashed per slot
        counts[L.aie_oracle_sample_row(pl, pm, 1, n, sampler_entry_rng(counter_rng(99, 0, t, 5), 3))] += 1
    assert counts[~allowed].sum() == 0, "a masked entry was drawn"
    w = np.exp(lg[allowed].astype(np.float64) - lg[allowed].max())
    prob = w / w.sum()
    exp = N * prob
    keep = exp >= 5
    left_out = float(prob[~keep].sum())
    assert left_out <= 0.01, "the cells left out of the chi-square hold %.3f of the mass" % left_out
    assert keep[-1], "the last entry's cell is part of the test"
    chi2 = float((((counts[allowed] - exp) ** 2) / exp)[keep].sum())
    dof = int(keep.sum()) - 1
    q = dof * (1 - 2 / (9 * dof) + 3.09 * math.sqrt(2 / (9 * dof))) ** 3  # Wilson-Hilferty, 99.9 %
    print("n = %d: chi-square %.1f, 99.9 %% quantile %.1f (%.2f of it), left-out mass %.4f, the last entry %d of %.0f expected" % (
        n, chi2, q, chi2 / q, left_out, counts[n - 1], exp[-1]))
    assert chi2 < q, (n, chi2, q, dof)
    # the last entry alone: a binomial count, the same 99.9 % (two-sided normal quantile 3.29)
    sd = math.sqrt(N * prob[-1] * (1 - prob[-1]))
    assert abs(counts[n - 1] - exp[-1]) <= 3.29 * sd, (n, counts[n - 1], exp[-1], sd)
