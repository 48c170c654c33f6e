"""Generalised advantage estimation, CPU side: the header's aie_gae_step (csrc/aie_trainer_math.h -- what aie_gae's kernel calls),
compiled here with the host C compiler (contraction off) and run down columns, against the plain NumPy float32 loop
(tests/gae_ref.py), bit for bit; and the two new exports of the built library with their ctypes bindings."""
import ctypes
import os
import subprocess
import tempfile

import numpy as np
import pytest

import gae_ref
from gae_ref import bits, f32
from helpers import ROOT

CSRC = os.path.join(ROOT, "ai-economist_amd", "csrc")

SHIM = r"""
#include "aie_trainer_math.h"
/* columns side by side: r, done [T][C], v [T + 1][C] -> adv, ret [T][C] */
void shim_gae(const float* r, const float* done, const float* v, long T, long C, float gamma, float lambda, float* adv, float* ret) {
  const float gl = aie_gae_gl(gamma, lambda);
  for (long c = 0; c < C; ++c) {
    float a_next = 0.0f;
    for (long t = T - 1; t >= 0; --t) {
      const float a = aie_gae_step(r[t * C + c], v[t * C + c], v[(t + 1) * C + c], a_next, done[t * C + c] > 0.5f, gamma, gl);
      adv[t * C + c] = a;
      ret[t * C + c] = aie_gae_return(a, v[t * C + c]);
      a_next = a;
    }
  }
}
"""


@pytest.fixture(scope="module")
def shim():
    with tempfile.TemporaryDirectory() as d:
        src, so = os.path.join(d, "shim.c"), os.path.join(d, "shim.so")
        with open(src, "w") as f:
            f.write(SHIM)
        subprocess.run(["gcc", "-O2", "-mfma", "-ffp-contract=off", "-shared", "-fPIC", "-I" + CSRC,
                        "-I" + os.path.join(ROOT, "include"), src, "-o", so, "-lm"], check=True)
        lib = ctypes.CDLL(so)
        fp = ctypes.POINTER(ctypes.c_float)
        lib.shim_gae.argtypes = [fp, fp, fp, ctypes.c_long, ctypes.c_long, ctypes.c_float, ctypes.c_float, fp, fp]
        yield lib


def c_gae(lib, r, done, v, gamma, lam):
    r, done, v = (np.ascontiguousarray(x, f32) for x in (r, done, v))
    T, C = r.shape
    adv, ret = np.empty((T, C), f32), np.empty((T, C), f32)
    p = lambda a: a.ctypes.data_as(ctypes.POINTER(ctypes.c_float))  # noqa: E731
    lib.shim_gae(p(r), p(done), p(v), T, C, gamma, lam, p(adv), p(ret))
    return adv, ret


COLUMNS = 37
GAMMA, LAM = 0.998, 0.98


def _case(T, p_done, seed):
    rng = np.random.RandomState(seed)
    r = rng.randn(T, COLUMNS).astype(f32)
    v = (rng.randn(T + 1, COLUMNS) * 10).astype(f32)
    done = (rng.rand(T, COLUMNS) < p_done).astype(f32)
    return r, done, v


@pytest.mark.parametrize("T", [1, 7, 200])
@pytest.mark.parametrize("p_done", [0.0, 0.2, 1.0])
def test_gae_step_equals_the_numpy_float32_loop(shim, T, p_done):
    r, done, v = _case(T, p_done, 10 * T + int(10 * p_done))
    for gamma, lam in ((GAMMA, LAM), (0.9, 0.5), (1.0, 1.0)):
        adv, ret = c_gae(shim, r, done, v, gamma, lam)
        want_adv, want_ret = gae_ref.gae(r, done, v, gamma, lam)
        assert np.array_equal(bits(adv), bits(want_adv)), (T, p_done, gamma, lam)
        assert np.array_equal(bits(ret), bits(want_ret)), (T, p_done, gamma, lam)
        assert np.isfinite(adv).all() and np.isfinite(ret).all()


@pytest.mark.parametrize("T", [1, 7, 200])
def test_done_at_the_last_step_ignores_the_bootstrap_value(shim, T):
    r, done, v = _case(T, 0.2, 500 + T)
    done[T - 1] = 1.0
    adv, ret = c_gae(shim, r, done, v, GAMMA, LAM)
    want_adv, want_ret = gae_ref.gae(r, done, v, GAMMA, LAM)
    assert np.array_equal(bits(adv), bits(want_adv)) and np.array_equal(bits(ret), bits(want_ret))
    v2 = v.copy()
    v2[T] = 12345.0  # the bootstrap row takes no part behind a done step
    adv2, ret2 = c_gae(shim, r, done, v2, GAMMA, LAM)
    assert np.array_equal(bits(adv2), bits(adv)) and np.array_equal(bits(ret2), bits(ret))
    assert np.array_equal(bits(adv[T - 1]), bits(r[T - 1] - v[T - 1]))


@pytest.mark.parametrize("T", [1, 7, 200])
@pytest.mark.parametrize("poison", [np.nan, np.inf, -np.inf])
def test_nothing_behind_a_done_step_leaks(shim, T, poison):
    """NaN and +-inf planted in V_{t+1} behind every done step (the restarted episode's value under auto-reset would sit
    there) and in the row-T bootstrap behind a done last step: outputs are finite and equal the unpoisoned run's wherever the
    poisoned value is not the step's own V_t."""
    r, done, v = _case(T, 0.2, 900 + T)
    done[T - 1] = 1.0
    clean_adv, clean_ret = c_gae(shim, r, done, v, GAMMA, LAM)
    vp = v.copy()
    vp[T][done[T - 1] > 0.5] = poison  # the bootstrap row: never anybody's own V_t
    adv, ret = c_gae(shim, r, done, vp, GAMMA, LAM)
    assert np.array_equal(bits(adv), bits(clean_adv)) and np.array_equal(bits(ret), bits(clean_ret))
    # V_{t+1} behind done steps inside the fragment is step t + 1's own V_t: poison it only where step t + 1 is not read as
    # an own value, i.e. compare against the reference on the same poisoned input and require the rows at and before the done
    # step to be clean
    if T > 1:
        vq = v.copy()
        t_idx, c_idx = np.nonzero(done[: T - 1] > 0.5)
        vq[t_idx + 1, c_idx] = poison
        adv, ret = c_gae(shim, r, done, vq, GAMMA, LAM)
        want_adv, want_ret = gae_ref.gae(r, done, vq, GAMMA, LAM)
        own = np.zeros((T, COLUMNS), bool)  # steps whose own V_t is poisoned: their outputs are poisoned by definition
        own[t_idx + 1, c_idx] = True
        reach = own.copy()                  # ... and the steps before them in the same episode
        for t in range(T - 2, -1, -1):
            reach[t] |= reach[t + 1] & ~(done[t] > 0.5)
        assert (~reach).any()
        assert np.array_equal(bits(adv[~reach]), bits(want_adv[~reach])) and np.array_equal(bits(ret[~reach]), bits(want_ret[~reach]))
        assert np.isfinite(adv[~reach]).all() and np.isfinite(ret[~reach]).all()
        done_rows = (done > 0.5) & ~own
        assert np.array_equal(bits(adv[done_rows]), bits((r - v[:T])[done_rows]))  # the done steps themselves: r - V, clean


def test_float32_is_the_right_width(shim):
    """Against the same loop in float64 the float32 recurrence is off by ~3e-7 of max|A| (T = 200, N(0,1) rewards, N(0,10^2)
    values).  The bound is the worst case of the arithmetic: a step makes five roundings (two products, three sums), each at
    most eps / 2 of an intermediate no larger than M = max|r| + 2 max|V| + max|A|, and an error made at step t reaches step
    t - k scaled by (gamma lambda)^k: at most 5 (eps / 2) M / (1 - gamma lambda) in all."""
    r, done, v = _case(200, 0.0, 7)
    adv, _ = c_gae(shim, r, done, v, GAMMA, LAM)
    a64 = np.zeros((200, COLUMNS))
    last = np.zeros(COLUMNS)
    r64, v64 = r.astype(np.float64), v.astype(np.float64)
    for t in range(199, -1, -1):
        last = r64[t] + GAMMA * v64[t + 1] - v64[t] + GAMMA * LAM * last
        a64[t] = last
    err = np.abs(adv - a64).max()
    M = np.abs(r64).max() + 2 * np.abs(v64).max() + np.abs(a64).max()
    bound = 5 * (np.finfo(f32).eps / 2) * M / (1 - GAMMA * LAM)
    print("float32 GAE against float64: %.2e of max|A| (bound %.2e)" % (err / np.abs(a64).max(), bound / np.abs(a64).max()))
    assert err <= bound


def test_library_exports_and_binds_the_two_calls():
    from ai_economist_amd import _build, _cabi

    lib = _cabi.bind(ctypes.CDLL(_build.build()))
    for sym in ("aie_gae", "aie_trajectory_store"):
        assert sym in _cabi.EXPORTED_SYMBOLS
        assert getattr(lib, sym).restype is ctypes.c_int
    assert len(lib.aie_gae.argtypes) == 14 and len(lib.aie_trajectory_store.argtypes) == 6
    assert ctypes.sizeof(_cabi.AieTrajSegment) == 32
    # no environment: refused before anything is touched
    assert lib.aie_gae(None, 1, None, 1, 0, None, None, 0.9, 0.9, None, None, None, None, None) == _cabi.E_INVALID
    assert lib.aie_trajectory_store(None, None, 1, 1, None, None) == _cabi.E_INVALID
