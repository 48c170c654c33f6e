"""Row lengths at the edges of the policy kernels' lane segments and 64-entry chunks: the case table of
tests/test_policy_row_edges_cpu.py (CPU) and tests/test_gpu_policy_row_edges.py (device).  No test functions here.

A row of `len` entries takes a segment of 16, 32 or 64 lanes (csrc/aie_trainer_math.h: aie_sampler_segment); rows of more
than 64 entries go to the generic kernels in chunks of 64.  The workloads' own rows (6, 12, 22, 50, 52, 148 entries) never
fill a segment to its last lane, never sit one entry over a segment size, and never end in a chunk of one entry.  The
configurations below do, with public configuration only:

    agents' single-action row    1 + (Build: 1) + (Gather: 4) + (auction: 4 (max_bid_ask + 1))
    planner, multi-action        n_brackets rows of n_rates + 1
    planner, single-action       one row of 1 + n_brackets n_rates
    n_rates                      the multiples of rate_disc from 0 to rate_max (rate_disc a power of two: exact)

Each case records the lengths it is built for and the sampler instance aie_capi.hip's aie_policy_sampler picks for them
(`lsh`: log2 of the lanes per row of a class; `generic`: the kernel for rows of any shape); the CPU test holds both to
mask_keys and aie_sampler_args_of, so the device tests run the instance they name.
"""
from helpers import C2

SEGMENTS = (16, 32, 64)


def segment(n):
    """aie_sampler_segment."""
    return 16 if n <= 16 else 32 if n <= 32 else 64


def _tax(disc, rate_max, **kw):
    return ["PeriodicBracketTax", dict(rate_disc=disc, rate_max=rate_max, period=10, **kw)]


def _cda(max_bid_ask):
    return ["ContinuousDoubleAuction", {"max_num_orders": 5, "max_bid_ask": max_bid_ask}]


BUILD, GATHER = ["Build", {}], ["Gather", {}]

# case -> (components, planner multi-action?, n_agents, agents' row, (planner rows, entries per row), what the case is for)
_TABLE = {
    "a14_p32": ([BUILD, _cda(1), GATHER, _tax(1 / 32, 30 / 32)], True, 5, 14, (7, 32), "fast (4,5): the planner's segment full"),
    "a17_p16": ([_cda(2), GATHER, _tax(1 / 16, 14 / 16)], True, 5, 17, (7, 16), "fast (5,4): one over 16; a full 16"),
    "a17_p17": ([_cda(2), GATHER, _tax(1 / 16, 15 / 16)], True, 5, 17, (7, 17), "fast (5,5)"),
    "a17_p64": ([_cda(2), GATHER, _tax(1 / 64, 62 / 64)], True, 5, 17, (7, 64), "fast (5,6): a full 64"),
    "a33_p16": ([_cda(6), GATHER, _tax(1 / 16, 14 / 16)], True, 4, 33, (7, 16), "fast (6,4): one over 32"),
    "a33_p33": ([_cda(6), GATHER, _tax(1 / 32, 31 / 32)], True, 4, 33, (7, 33), "fast (6,6)"),
    "a62_p64": ([BUILD, _cda(13), GATHER, _tax(1 / 8, 1.0)], False, 4, 62, (1, 64), "fast (6,6): a lone full row"),
    "a65_p65": ([_cda(14), GATHER, _tax(1 / 64, 63 / 64)], True, 4, 65, (7, 65), "generic: a second chunk of one entry, both classes"),
    "a6_p65": ([BUILD, GATHER, _tax(1 / 16, 15 / 16, n_brackets=4, bracket_spacing="linear")], False, 4, 6, (1, 65), "generic planner"),
    "a6_p129": ([BUILD, GATHER, _tax(1 / 16, 15 / 16, n_brackets=8, bracket_spacing="linear")], False, 4, 6, (1, 129),
                "generic: two full chunks and one entry"),
}
CASES = list(_TABLE)


class Case:
    def __init__(self, name):
        comps, multi_p, n, len_a, (rows_p, len_p), self.what = _TABLE[name]
        self.name, self.n, self.len_a, self.rows_p, self.len_p, self.multi_p = name, n, len_a, rows_p, len_p, multi_p
        self.cfg = dict(C2, episode_length=30, components=comps, n_agents=n, multi_action_mode_agents=False,
                        multi_action_mode_planner=multi_p)
        # aie_policy_sampler: the generic kernel when a row is longer than 64 entries (single-action agents: never ragged)
        self.generic = len_a > 64 or len_p > 64
        self.lsh = tuple({16: 4, 32: 5, 64: 6}[segment(ln)] for ln in (len_a, len_p))  # (agents, planner)
        # the PPO loss: a class whose actors have one slot of at most 64 entries takes ppo_fast<lsh>, else ppo_generic
        self.ppo_generic = (len_a > 64, rows_p > 1 or len_p > 64)

    def rows(self):
        """{"a": [(offset, length)], "p": [...]}: the slots inside one actor's logits (test_gpu_policy_evaluate._rows)."""
        return {"a": [(0, self.len_a)], "p": [(s * self.len_p, self.len_p) for s in range(self.rows_p)]}


def case(name):
    return Case(name)


FAST_INSTANCES = sorted({Case(c).lsh for c in CASES if not Case(c).generic})


def edge_logits(n, rng, quarter_masked=True):
    """(logits, mask) of one row of n entries for the distribution test: the largest logit on the LAST entry, a quarter of
    the other entries masked, the rest within 2.5 of the maximum -- at 20 000 draws every allowed entry is then expected
    at least 5 times up to 129 entries (e^-2.5 / 129 x 20 000 > 12), so no cell is left out of the chi-square."""
    import numpy as np

    lg = rng.uniform(-2.5, -0.5, n).astype(np.float32)
    lg[n - 1] = 0.0
    mask = np.ones(n, np.float32)
    if quarter_masked and n > 1:
        off = rng.permutation(n - 1)[: (n - 1) // 4]
        mask[off] = 0.0
    return lg, mask
