"""Rich states of the gather-trade-build kernels: the corners a uniform random policy never reaches (high tax brackets,
busy auctions, full books, crowded maps, extreme coin), and how the tests get there.

  census(before, after, actions, env)   named reach conditions of ONE step, from state tensors only (NumPy; oracle and
                                        device tensors alike) -- what keeps the GPU tests from being vacuous
  policy_actions(kind, env, ...)        closed-loop scripted policies (builder / market / mix): deterministic functions
                                        of the action masks, a seed and the step number
  rich_state(env, base, kind, rng)      injected states in the load_state format, with hand-built order books
  assert_invariants(state, env)         everything a state of the reference always satisfies

No test functions here: tests/test_rich_states_cpu.py checks on the oracle alone that every scenario below reaches the
conditions it declares (and, reference-marked, pins the policy rollouts to the live reference);
tests/test_gpu_rich_states.py runs the same scenarios on the device against the oracle.

Two readings the condition list needs:
  * an agent's orders for one resource, bids and asks TOGETHER, are limited by max_num_orders
    (continuous_double_auction.py: n_orders[resource][agent] guards create_bid and create_ask alike), so the bid book
    and the ask book of one resource hold at most M = n_agents * max_num_orders orders between them: "book at
    capacity" is one side holding all M (`cda_bid_book_full`, `cda_ask_book_full`), which is also where the kernels'
    book arrays are indexed up to their end;
  * a mask-respecting policy is never refused an order in single-action mode (the masks are exactly create_bid's and
    create_ask's conditions); the refusals are reached by agents that post several sub-actions in one step
    (multi-action mode: the second order of a step meets the quota / the coin the first one used; a build uses the
    resource an ask wanted) and by `pushy` agents that ignore the auction's masks, which the reference accepts and
    refuses order by order.
"""
import numpy as np

from helpers import GTB, C2, _components_with

AIE_COMP = {1: "Build", 2: "ContinuousDoubleAuction", 3: "Gather", 4: "PeriodicBracketTax", 9: "WealthRedistribution"}
PLANNER_REWARD_TYPES = ("coin_eq_times_productivity", "inv_income_weighted_coin_endowments", "inv_income_weighted_utility")

STATE_KEYS = ("inv_coin", "esc_coin", "inv_res", "esc_res", "labor", "util", "loc_r", "loc_c", "house_owner", "cell_flags",
              "stone", "wood", "build_payment", "cda_n_bids", "cda_n_asks", "cda_bids", "cda_asks", "cda_n_orders",
              "cda_bid_hist", "cda_ask_hist", "tax_cycle_pos", "tax_last_completions", "tax_rate_idx", "tax_last_coin",
              "tax_last_income", "metrics_cda_trades", "metrics_tax_paid_sum", "metrics_tax_days", "timestep",
              "regen_src_n", "regen_src_list", "error_flags")


def snapshot(tensors, sl=None):
    """Copies of the state tensors the census reads, as NumPy arrays (oracle arrays or device tensors)."""
    out = {}
    for k in STATE_KEYS:
        if k in tensors:
            v = tensors[k]
            v = v.cpu().numpy() if hasattr(v, "cpu") else np.asarray(v)
            out[k] = np.array(v if sl is None else v[sl])
    return out


class Info:
    """What the census, the policies and the state builder need to know about a configuration."""

    def __init__(self, env):
        c = env.build_config()
        self.n, self.H, self.W = int(c.n_agents), int(c.world_h), int(c.world_w)
        self.comps = [AIE_COMP.get(int(x), "?") for x in list(c.components)[: c.n_components]]
        self.has_cda = "ContinuousDoubleAuction" in self.comps
        self.has_tax = "PeriodicBracketTax" in self.comps
        self.has_build = "Build" in self.comps
        self.maxo, self.P, self.dur = int(c.cda_max_num_orders), int(c.cda_max_bid_ask) + 1, int(c.cda_order_duration)
        self.M = self.n * self.maxo if self.has_cda else 0
        self.NB = int(c.tax_n_brackets) if self.has_tax else 0
        self.cut = np.array(list(c.tax_bracket_cutoffs)[: self.NB], np.float64)
        self.period, self.tax_model = int(c.tax_period), int(c.tax_model)  # 0: model_wrapper
        self.disc = np.array(list(c.tax_disc_rates)[: c.tax_n_disc_rates], np.float64)
        self.fixed = np.array(list(c.tax_fixed_rates)[: self.NB], np.float64)
        self.annealing = bool(c.tax_annealing)
        self.warmup, self.slope, self.rate_max = float(c.tax_annealing_warmup), float(c.tax_annealing_slope), float(c.tax_rate_max)
        self.tax_disabled = bool(c.tax_disable)
        self.multi, self.multi_p = bool(c.multi_action_mode_agents), bool(c.multi_action_mode_planner)
        self.planner_reward_type = PLANNER_REWARD_TYPES[int(c.planner_reward_type)]
        self.episode_length = int(c.episode_length)
        names_a, names_p = env.action_subspace_names()
        self.subs = []  # (slot, choices): slot "build", "move", ("buy", r), ("sell", r)
        for name, d in names_a:
            if name == "Build":
                slot = "build"
            elif name == "Gather":
                slot = "move"
            else:
                side, res = name.split(".")[1].split("_")
                slot = (side.lower(), ("Stone", "Wood").index(res))
            self.subs.append((slot, int(d)))
        self.subs_p = [int(d) for _, d in names_p]
        # single-action mode: one index over [NO-OP, subspace 0, subspace 1, ...]; multi-action: one column per subspace
        self.base, self.moff, b, o = {}, {}, 1, 0
        for s, (slot, d) in enumerate(self.subs):
            self.base[slot] = b
            self.moff[slot] = b if not self.multi else o + 1  # mask entry of the subspace's first choice
            b += d
            o += d + 1
        self.col = {slot: s for s, (slot, _) in enumerate(self.subs)}
        self.dim = dict(self.subs)

    def before(self, a, b):
        """Component a steps ahead of component b (or b is absent)."""
        return a in self.comps and (b not in self.comps or self.comps.index(a) < self.comps.index(b))

    def annealed_limit(self, completions, final_max):
        pv = np.clip(self.slope * (np.asarray(completions, np.float64) - self.warmup), 0.0, 1.0)
        return pv * final_max

    def rates(self, t):
        """[E, NB] marginal rates in force (curr_marginal_rates): chosen or fixed, under the annealed limit."""
        if self.tax_model == 0:
            r = self.disc[t["tax_rate_idx"]]
        else:
            r = np.broadcast_to(self.fixed, (len(t["tax_cycle_pos"]), self.NB)).copy()
        if self.annealing and self.tax_model != 0:
            r = np.minimum(r, self.annealed_limit(t["tax_last_completions"], self.rate_max)[:, None])
        return r

    def uncapped_rates(self, t):
        if self.tax_model == 0:
            return self.disc[t["tax_rate_idx"]]
        return np.broadcast_to(self.fixed, (len(t["tax_cycle_pos"]), self.NB))


def decode_actions(info, a):
    """a: int [E, n, width] -> {slot: [E, n] choice, 0 = none} (base_agent.py parse_actions)."""
    a = np.asarray(a)
    if a.ndim == 2:
        a = a[:, :, None]
    out = {}
    for slot, d in info.subs:
        if info.multi:
            v = a[:, :, info.col[slot]]
            out[slot] = np.where((v >= 0) & (v <= d), v, 0)
        else:
            v = a[:, :, 0] - info.base[slot] + 1
            out[slot] = np.where((v >= 1) & (v <= d), v, 0)
    return out


def encode_actions(info, ch, E):
    """{slot: [E, n] choice} -> the action buffer (single-action mode: the LAST listed non-zero slot wins)."""
    if info.multi:
        a = np.zeros((E, info.n, max(1, len(info.subs))), np.int32)
        for slot, v in ch.items():
            a[:, :, info.col[slot]] = v
    else:
        a = np.zeros((E, info.n, 1), np.int32)
        for slot, v in ch.items():
            a[:, :, 0] = np.where(v > 0, info.base[slot] + v - 1, a[:, :, 0])
    return a


# ----------------------------------------------------------------------------------------------------------------
# census
# ----------------------------------------------------------------------------------------------------------------
ORD_AGENT = lambda o: o & 0xff  # noqa: E731
ORD_PRICE = lambda o: (o >> 8) & 0xff  # noqa: E731
ORD_LIFE = lambda o: (o >> 16) & 0xffff  # noqa: E731


def _match(bids, asks, n):
    """continuous_double_auction.py match_orders for one resource.  bids / asks: lists of (agent, price, lifetime) in
    arrival order.  Returns (trades, bids left, asks left); a trade is (seller, buyer, ask, bid, price, at_ask)."""
    bids = sorted(bids, key=lambda b: (b[1], b[2]), reverse=True)
    asks = sorted(asks, key=lambda a: (a[1], -a[2]))
    possible = [True] * n
    trades = []
    keep = True
    while any(possible) and keep:
        ib = ia = 0
        while True:
            if ib >= len(bids):
                keep = False
                break
            buyer = bids[ib][0]
            if not possible[buyer]:
                ib += 1
            elif ia >= len(asks):
                possible[buyer] = False
                break
            elif asks[ia][0] == buyer:
                ia += 1
            elif bids[ib][1] < asks[ia][1]:
                possible[buyer] = False
                break
            else:
                b, a = bids.pop(ib), asks.pop(ia)
                at_ask = b[2] <= a[2]
                trades.append((a[0], buyer, a[1], b[1], a[1] if at_ask else b[1], at_ask))
                break
    return trades, bids, asks


TAX_CONDITIONS = ("tax_every_bracket", "tax_income_on_cutoff", "tax_negative_income", "tax_tiny_income",
                  "tax_due_capped_with_escrow", "tax_annealed_cap_in_high_bracket", "tax_nb_ge8_ragged",
                  "tax_nb_multiple_of_8")
CDA_CONDITIONS = ("cda_n_trades_in_a_step", "cda_bid_book_full", "cda_ask_book_full", "cda_refused_at_quota",
                  "cda_bid_refused_for_coin", "cda_bid_accepted_at_coin_equal_price", "cda_ask_refused_without_inventory",
                  "cda_equal_price_other_lifetime", "cda_equal_price_equal_lifetime", "cda_buyer_crosses_only_own_asks",
                  "cda_trade_at_ask_price", "cda_trade_at_bid_price", "cda_expiry_in_full_book", "cda_trade_at_price_0",
                  "cda_trade_at_max_price", "cda_bid_and_ask_same_step")
OTHER_CONDITIONS = ("build_with_exact_resources", "houses_ge_10", "all_moves_blocked", "inventory_ge_256",
                    "coin_span_1e-3_1e5", "all_agents_equal_coin", "one_agent_holds_all_coin", "total_coin_zero",
                    "all_utilities_negative") + tuple("planner_reward_" + k for k in PLANNER_REWARD_TYPES)
CONDITIONS = TAX_CONDITIONS + tuple("%s[%s]" % (k, r) for k in CDA_CONDITIONS for r in ("Stone", "Wood")) + OTHER_CONDITIONS


def census(before, after, actions, env, info=None):
    """{condition: bool} for one step of E replicas.  before / after: snapshot()s around the step, actions: the agents'
    action buffer.  The auction's conditions come from replaying create_bid / create_ask / match_orders in Python on the
    state before the step; the replay's surviving books are checked against the state after it, so a condition is
    never reported for a step this module misread.  `tax_bracket_counts` (int [NB]) is extra: Reach adds it up."""
    info = info or Info(env)
    n, E = info.n, len(before["inv_coin"])
    act = decode_actions(info, actions)
    out = {k: False for k in CONDITIONS}
    out["tax_bracket_counts"] = np.zeros(max(info.NB, 1), np.int64)
    out["planner_reward_" + info.planner_reward_type] = True

    # ---- Build: which agents built (a house more on the map)
    owners_b, owners_a = before["house_owner"].reshape(E, -1), after["house_owner"].reshape(E, -1)
    built = np.stack([(owners_a == i).sum(1) - (owners_b == i).sum(1) for i in range(n)], 1) > 0  # [E, n]
    build_first = info.has_build and all(info.before("Build", x) for x in ("ContinuousDoubleAuction", "Gather"))
    if info.has_build and build_first:
        out["build_with_exact_resources"] = bool((built & (before["inv_res"][:, 0] == 1) & (before["inv_res"][:, 1] == 1)).any())
    out["houses_ge_10"] = bool(((owners_a >= 0).sum(1) >= 10).any())
    out["inventory_ge_256"] = bool(((after["inv_res"] >= 256) | (before["inv_res"] >= 256)).any())

    # ---- Move: all four neighbours closed by the edge, water or somebody else's house
    lr, lc = after["loc_r"], after["loc_c"]
    closed = np.ones((E, n), bool)
    ee = np.arange(E)[:, None]
    for dr, dc in ((0, -1), (0, 1), (-1, 0), (1, 0)):
        r, c = lr + dr, lc + dc
        inside = (r >= 0) & (r < info.H) & (c >= 0) & (c < info.W)
        rr, cc = np.clip(r, 0, info.H - 1), np.clip(c, 0, info.W - 1)
        own = after["house_owner"][ee, rr, cc]
        water = (after["cell_flags"][ee, rr, cc] & 1) > 0
        closed &= ~inside | water | ((own >= 0) & (own != np.arange(n)[None, :]))
    out["all_moves_blocked"] = bool(closed.any())

    # ---- rewards
    coin = after["inv_coin"] + after["esc_coin"]
    pos = np.where(coin > 0, coin, np.inf)
    out["coin_span_1e-3_1e5"] = bool(((pos.min(1) <= 1e-3) & (coin.max(1) >= 1e5)).any())
    tot = coin.sum(1)
    out["all_agents_equal_coin"] = bool(((coin == coin[:, :1]).all(1) & (tot > 0)).any())
    out["one_agent_holds_all_coin"] = bool((((coin > 0).sum(1) == 1) & ((coin == 0).sum(1) == n - 1)).any())
    out["total_coin_zero"] = bool((coin == 0).all(1).any())
    out["all_utilities_negative"] = bool((after["util"][:, :n] < 0).all(1).any())

    # ---- PeriodicBracketTax: replicas whose step was a tax day
    if info.has_tax and not info.tax_disabled:
        day = after["metrics_tax_days"] > before["metrics_tax_days"]
        if day.any():
            inc = after["tax_last_income"][day]  # [D, n]
            nonneg = inc >= 0
            b = np.clip(np.searchsorted(info.cut, inc, side="right") - 1, 0, info.NB - 1)
            b = np.where(nonneg, b, 0)
            out["tax_bracket_counts"] = np.bincount(b.reshape(-1), minlength=info.NB).astype(np.int64)
            out["tax_income_on_cutoff"] = bool(np.isin(inc, info.cut[1:]).any())
            out["tax_negative_income"] = bool((inc < 0).any())
            out["tax_tiny_income"] = bool(((inc > 0) & (inc < 1e-6)).any())
            out["tax_nb_ge8_ragged"] = info.NB >= 8 and info.NB % 8 != 0
            out["tax_nb_multiple_of_8"] = info.NB >= 8 and info.NB % 8 == 0
            rates = info.rates(after)[day]  # [D, NB] (rate indices change at period starts, ahead of the tax day's levy)
            size = np.append(np.diff(info.cut), np.inf)
            binned = np.minimum(size[None, None, :], np.maximum(inc[:, :, None] - info.cut[None, None, :], 0.0))
            due = (rates[:, None, :] * binned).sum(2)
            paid = (after["metrics_tax_paid_sum"] - before["metrics_tax_paid_sum"])[day]
            esc = np.minimum(before["esc_coin"], after["esc_coin"])[day]
            out["tax_due_capped_with_escrow"] = bool(((paid < due * (1 - 1e-9)) & (due > 0) & (esc > 0)).any())
            if info.annealing:
                cap_max = info.rate_max if info.tax_model != 0 else np.abs(info.disc).max()
                lim = info.annealed_limit(after["tax_last_completions"][day], cap_max)  # [D]
                unc = info.uncapped_rates(after)[day]  # [D, NB]
                hit = (unc > lim[:, None])[np.arange(len(b))[:, None], b] & (b >= 3) & nonneg
                out["tax_annealed_cap_in_high_bracket"] = bool(hit.any())

    # ---- ContinuousDoubleAuction: replay the step's orders
    if info.has_cda and not (info.before("PeriodicBracketTax", "ContinuousDoubleAuction")
                             or info.before("WealthRedistribution", "ContinuousDoubleAuction")
                             or info.before("Gather", "ContinuousDoubleAuction")):
        pay = np.where(built, before["build_payment"], 0.0) if info.before("Build", "ContinuousDoubleAuction") else 0.0
        spent = built.astype(np.int64) if info.before("Build", "ContinuousDoubleAuction") else 0
        coin_now = before["inv_coin"] + pay  # [E, n]
        inv_now = before["inv_res"] - (spent[:, None, :] if info.has_build else 0)  # [E, 2, n]
        no_now = before["cda_n_orders"].copy()
        new_b = np.zeros((E, 2, n), np.int64) - 1  # price of the accepted bid / ask, -1: none
        new_a = np.zeros((E, 2, n), np.int64) - 1
        sold = after["metrics_cda_trades"][:, 0, :, :, 0].sum(2) - before["metrics_cda_trades"][:, 0, :, :, 0].sum(2)  # [E, 2]
        for r in range(2):
            R = ("Stone", "Wood")[r]
            buy, sell = act.get(("buy", r)), act.get(("sell", r))
            for i in range(n):
                if buy is not None:
                    want = buy[:, i] > 0
                    price = buy[:, i] - 1
                    quota = no_now[:, r, i] < info.maxo
                    ok = want & quota & ~(coin_now[:, i] < price)
                    out["cda_refused_at_quota[%s]" % R] |= bool((want & ~quota).any())
                    out["cda_bid_refused_for_coin[%s]" % R] |= bool((want & quota & ~ok).any())
                    out["cda_bid_accepted_at_coin_equal_price[%s]" % R] |= bool((ok & (coin_now[:, i] == price) & (price > 0)).any())
                    new_b[:, r, i] = np.where(ok, price, -1)
                    no_now[:, r, i] += ok
                    coin_now[:, i] -= np.where(ok, np.minimum(coin_now[:, i], price), 0.0)
                if sell is not None:
                    want = sell[:, i] > 0
                    price = sell[:, i] - 1
                    quota = no_now[:, r, i] < info.maxo
                    ok = want & quota & (inv_now[:, r, i] > 0)
                    out["cda_refused_at_quota[%s]" % R] |= bool((want & ~quota).any())
                    out["cda_ask_refused_without_inventory[%s]" % R] |= bool((want & quota & ~ok).any())
                    new_a[:, r, i] = np.where(ok, price, -1)
                    no_now[:, r, i] += ok
                    inv_now[:, r, i] -= ok
            out["cda_bid_and_ask_same_step[%s]" % R] = bool(((new_b[:, r] >= 0) & (new_a[:, r] >= 0)).any())
            out["cda_n_trades_in_a_step[%s]" % R] = bool((sold[:, r] >= n).any())
            out["cda_bid_book_full[%s]" % R] = bool((after["cda_n_bids"][:, r] == info.M).any())
            out["cda_ask_book_full[%s]" % R] = bool((after["cda_n_asks"][:, r] == info.M).any())
            for e in range(E):
                nb0, na0 = int(before["cda_n_bids"][e, r]), int(before["cda_n_asks"][e, r])
                fresh = (new_b[e, r] >= 0).any() or (new_a[e, r] >= 0).any()
                if not fresh and nb0 == 0 and na0 == 0:
                    continue
                bids = [(int(ORD_AGENT(o)), int(ORD_PRICE(o)), int(ORD_LIFE(o))) for o in before["cda_bids"][e, r, :nb0]]
                asks = [(int(ORD_AGENT(o)), int(ORD_PRICE(o)), int(ORD_LIFE(o))) for o in before["cda_asks"][e, r, :na0]]
                bids += [(i, int(new_b[e, r, i]), 0) for i in range(n) if new_b[e, r, i] >= 0]
                asks += [(i, int(new_a[e, r, i]), 0) for i in range(n) if new_a[e, r, i] >= 0]
                for book in (bids, asks):
                    seen = {}
                    for ag, pr, life in book:
                        for ag2, life2 in seen.get(pr, ()):
                            if ag2 != ag:
                                out["cda_equal_price_%s_lifetime[%s]" % ("equal" if life2 == life else "other", R)] = True
                        seen.setdefault(pr, []).append((ag, life))
                if fresh:
                    for i in range(n):
                        mine = [b[1] for b in bids if b[0] == i]
                        if mine and any(a[0] == i and a[1] <= max(mine) for a in asks) \
                                and not any(a[0] != i and a[1] <= max(mine) for a in asks):
                            out["cda_buyer_crosses_only_own_asks[%s]" % R] = True
                trades, bids, asks = _match(bids, asks, n)
                assert len(trades) == int(sold[e, r]), "census replay: replica %d %s: %d trades, the state says %d" % (
                    e, R, len(trades), int(sold[e, r]))
                for _, _, ask, bid, price, at_ask in trades:
                    if ask != bid:
                        out["cda_trade_at_%s_price[%s]" % ("ask" if at_ask else "bid", R)] = True
                    out["cda_trade_at_price_0[%s]" % R] |= price == 0
                    out["cda_trade_at_max_price[%s]" % R] |= price == info.P - 1
                for side, book, key in (("bid", bids, "cda_n_bids"), ("ask", asks, "cda_n_asks")):
                    left = [o for o in book if o[2] + 1 <= info.dur]
                    assert len(left) == int(after[key][e, r]), "census replay: replica %d %s %ss: %d left, the state says %d" % (
                        e, R, side, len(left), int(after[key][e, r]))
                    if len(book) == info.M and len(left) < len(book):
                        out["cda_expiry_in_full_book[%s]" % R] = True
    return out


class Reach:
    """Union of census() results over the steps of a scenario."""

    def __init__(self):
        self.flags, self.brackets = {k: False for k in CONDITIONS}, None

    def add(self, c):
        for k in CONDITIONS:
            self.flags[k] = self.flags[k] or bool(c[k])
        b = c["tax_bracket_counts"]
        if b.sum():
            self.brackets = b if self.brackets is None else self.brackets + b

    def result(self):
        out = dict(self.flags)
        out["tax_every_bracket"] = self.brackets is not None and bool((self.brackets > 0).all())
        return out

    def reached(self):
        return sorted(k for k, v in self.result().items() if v)


# ----------------------------------------------------------------------------------------------------------------
# closed-loop scripted policies
# ----------------------------------------------------------------------------------------------------------------
POLICIES = ("builder", "market", "mix")


def _allowed(info, masks_a, slot):
    o, d = info.moff[slot], info.dim[slot]
    return np.asarray(masks_a)[:, :, o: o + d] > 0.5


def _pick(rs, allowed, prefer=None):
    """A random allowed choice per agent (1-based, 0 where nothing is allowed); `prefer`: choices (0-based) tried first."""
    score = rs.rand(*allowed.shape) + 1e-3
    if prefer is not None:
        w = np.zeros(allowed.shape[-1])
        w[[p for p in prefer if p < allowed.shape[-1]]] = 4.0
        score = score + w
    score = score * allowed
    return np.where(allowed.any(-1), score.argmax(-1) + 1, 0)


def policy_actions(kind, env, masks_a, masks_p, seed, t, info=None, pushy=None):
    """Actions of the scripted policy `kind` for step t (0-based, counted from the episode's reset): a deterministic
    function of the masks, the seed and t.  Returns (a int32 [E, n, width], p int32 [E, width_p]).

    builder  builds wherever the mask allows it, otherwise walks (and so gathers)
    market   an order book script on few prices, so that ties and crossings occur: the first max_num_orders steps
             everybody bids for Stone at price 0, the next max_num_orders steps for Wood (full bid books, which expire
             whole order_duration steps later), then cycles of 20 steps, alternating between the resources -- resting
             asks at 6 / 7 / max and resting bids at 3 / 4, a step in which everybody bids the maximum, one in which
             everybody asks 0, one in which half bid 0 and half ask 0 -- with walks in between
    mix      builder and market agents side by side (by agent index and step)
    pushy    bool [E, n] (or None): these agents take the market's orders whatever the auction's masks say."""
    info = info or Info(env)
    masks_a = np.asarray(masks_a)
    E, n = masks_a.shape[0], info.n
    rs = np.random.RandomState((int(seed) * 1000003 + int(t) * 7919 + POLICIES.index(kind)) % (2 ** 31))
    ch = {}
    idx = np.arange(n)[None, :] + np.zeros((E, 1), np.int64)
    u = rs.rand(E, n)
    move = np.zeros((E, n), np.int64)
    if "move" in info.dim:  # walks keep a direction for a few steps (they cover more ground than a random walk)
        ok = _allowed(info, masks_a, "move")
        ahead = (idx + t // 6 + seed) % 4
        move = np.where(np.take_along_axis(ok, ahead[:, :, None], 2)[:, :, 0] & (u < 0.8), ahead + 1, _pick(rs, ok))
    can_build = _allowed(info, masks_a, "build")[:, :, 0] if "build" in info.dim else np.zeros((E, n), bool)
    if kind == "builder":
        is_builder = np.ones((E, n), bool)
    elif kind == "market":
        is_builder = np.zeros((E, n), bool)
    else:
        is_builder = ((idx + (t // 40)) % 2) == 0
    orders = {}
    if info.has_cda:
        P = info.P
        want = {slot: np.zeros((E, n), np.int64) for slot in info.dim if isinstance(slot, tuple)}
        c, r_cycle = (t - 2 * info.maxo) % 20, ((t - 2 * info.maxo) // 20) % 2
        r_step = rs.randint(0, 2, size=(E, n))
        everyone = np.ones((E, n), bool)

        def put(side, sel_r, who, prefer):
            for r in range(2):
                slot = (side, r)
                ok = _allowed(info, masks_a, slot)
                if pushy is not None:
                    ok = ok | pushy[:, :, None]
                v = _pick(rs, ok & np.isin(np.arange(P), prefer)[None, None, :], prefer)
                want[slot] = np.where(who & (sel_r == r) & (v > 0), v, want[slot])

        if t < 2 * info.maxo:
            put("buy", np.full((E, n), t // info.maxo), everyone, [0])
        elif c == 12:
            put("buy", np.full((E, n), r_cycle), everyone, [P - 1])
        elif c == 14:
            put("sell", np.full((E, n), r_cycle), everyone, [0])
        elif c == 16:
            rr = np.full((E, n), r_cycle)
            put("buy", rr, idx % 2 == 0, [0])
            put("sell", rr, idx % 2 == 1, [0])
        else:
            trade = u < (0.75 if info.multi else 0.45)
            if pushy is not None:
                trade = trade | pushy
            seller = rs.rand(E, n) < 0.6
            put("sell", r_step, trade & seller, [6, 7, P - 1])
            put("buy", r_step, trade & ~seller, [3, 4])
            if info.multi:  # a second order in the same step: the other side of the same resource, or the other resource
                both = rs.rand(E, n) < 0.5
                put("buy", r_step, trade & seller & both, [3, 4])
                put("sell", 1 - r_step, trade & ~seller & both, [6, 7])
                put("buy", 1 - r_step, trade & ~seller & ~both & (rs.rand(E, n) < 0.5), [4, P - 1])
        orders = want
    if info.multi:
        for slot, v in orders.items():
            ch[slot] = np.where(is_builder, 0, v)
        if "build" in info.dim:
            ch["build"] = np.where(is_builder | (kind != "market"), can_build.astype(np.int64), 0)
        if "move" in info.dim:
            ch["move"] = np.where(rs.rand(E, n) < 0.7, move, 0)
    else:
        traded = np.zeros((E, n), bool)
        if "move" in info.dim:
            ch["move"] = np.where(rs.rand(E, n) < 0.9, move, 0)
        for slot, v in orders.items():
            v = np.where(is_builder | traded, 0, v)
            traded |= v > 0
            ch[slot] = v
        if "build" in info.dim:
            ch["build"] = np.where(is_builder & can_build, 1, 0)
    a = encode_actions(info, ch, E)
    # planner: a random allowed rate per bracket (the masks open at period starts, under the annealed limit)
    wp = max(1, len(info.subs_p)) if info.multi_p else 1
    p = np.zeros((E, wp), np.int32)
    if info.subs_p and masks_p is not None:
        mp = np.asarray(masks_p) > 0.5
        if info.multi_p:
            o = 0
            for b, d in enumerate(info.subs_p):
                p[:, b] = _pick(rs, mp[:, o + 1: o + 1 + d][:, None, :])[:, 0]
                o += d + 1
        else:
            p[:, 0] = _pick(rs, mp[:, None, 1:])[:, 0]
    return a, p


# ----------------------------------------------------------------------------------------------------------------
# invariants of a reference state
# ----------------------------------------------------------------------------------------------------------------
def assert_invariants(state, env, info=None, where="state", source_list=False):
    """What a state of the reference satisfies after any step (and the kernels rely on), for ONE replica's state dict:
    books sorted the way match_orders left them (bids by (price, lifetime) descending, asks by price ascending then
    lifetime descending), lifetimes in 1 .. order_duration, no bid of one agent at or above an ask of another
    (match_orders ends only when every buyer's best bid is below the cheapest foreign ask), escrows / n_orders /
    order histograms equal to the books, every agent's orders within max_num_orders, agents on distinct cells that are
    neither water nor another agent's house, houses only on cells without resources or source blocks
    (Build.agent_can_build; landmarks never regrow there because regeneration needs a source block), tax_cycle_pos in
    1 .. period and -- source_list=True, device states only: the restatement regenerates from the planes and leaves
    the field empty -- the regeneration's source list equal to the source planes."""
    info = info or Info(env)
    n = info.n
    s = {k: np.asarray(v) for k, v in state.items()}
    if "water" in s:
        water, ssrc, wsrc = s["water"] > 0, s["stone_src"] > 0, s["wood_src"] > 0
    else:
        water, ssrc, wsrc = (s["cell_flags"] & 1) > 0, (s["cell_flags"] & 2) > 0, (s["cell_flags"] & 4) > 0
    cells = list(zip(s["loc_r"].tolist(), s["loc_c"].tolist()))
    assert len(set(cells)) == n, "%s: two agents on one cell" % where
    for i, (r, c) in enumerate(cells):
        assert 0 <= r < info.H and 0 <= c < info.W and not water[r, c], "%s: agent %d off the map or on water" % (where, i)
        assert s["house_owner"][r, c] in (-1, i), "%s: agent %d on a foreign house" % (where, i)
    house = s["house_owner"] >= 0
    assert (s["house_owner"] < n).all()
    assert not (house & ((s["stone"] > 0) | (s["wood"] > 0) | water | ssrc | wsrc)).any(), "%s: a house on a resource / source / water cell" % where
    assert not ((s["stone"] > 0) & ~ssrc).any() and not ((s["wood"] > 0) & ~wsrc).any(), "%s: a resource off its source blocks" % where
    assert (s["inv_res"] >= 0).all() and (s["esc_res"] >= 0).all() and (s["esc_coin"] >= 0).all(), "%s: a negative holding" % where
    # (WealthRedistribution sets inventory coin to the equal share MINUS the agent's escrow: negative where the escrow is larger)
    assert "WealthRedistribution" in info.comps or (s["inv_coin"] >= 0).all(), "%s: negative coin" % where
    if info.has_cda:
        esc_coin, esc_res = np.zeros(n), np.zeros((2, n), np.int64)
        n_orders = np.zeros((2, n), np.int64)
        hist = {"bids": np.zeros((2, n, info.P), np.int64), "asks": np.zeros((2, n, info.P), np.int64)}
        for r in range(2):
            books = {}
            for side in ("bids", "asks"):
                k = int(s["cda_n_" + side][r])
                assert 0 <= k <= info.M
                book = [(int(ORD_AGENT(o)), int(ORD_PRICE(o)), int(ORD_LIFE(o))) for o in s["cda_" + side][r, :k]]
                books[side] = book
                key = (lambda o: (-o[1], -o[2])) if side == "bids" else (lambda o: (o[1], -o[2]))
                assert [key(o) for o in book] == sorted(key(o) for o in book), "%s: %s of resource %d out of order" % (where, side, r)
                for ag, pr, life in book:
                    assert 0 <= ag < n and 0 <= pr < info.P and 1 <= life <= info.dur, "%s: order %r" % (where, (ag, pr, life))
                    n_orders[r, ag] += 1
                    hist[side][r, ag, pr] += 1
                    if side == "bids":
                        esc_coin[ag] += pr
                    else:
                        esc_res[r, ag] += 1
            for ag, pr, _ in books["bids"]:
                assert not any(a2 != ag and pa <= pr for a2, pa, _ in books["asks"]), "%s: a bid crosses a foreign ask" % where
        assert np.array_equal(n_orders, s["cda_n_orders"]) and (n_orders <= info.maxo).all(), "%s: n_orders" % where
        assert np.array_equal(hist["bids"], s["cda_bid_hist"]) and np.array_equal(hist["asks"], s["cda_ask_hist"]), "%s: order histograms" % where
        assert np.array_equal(esc_res, s["esc_res"]), "%s: resource escrow" % where
        assert np.array_equal(esc_coin, s["esc_coin"]), "%s: coin escrow" % where
    else:
        assert not s["esc_coin"].any() and not s["esc_res"].any()
    if info.has_tax:
        assert 1 <= int(s["tax_cycle_pos"]) <= info.period, "%s: tax_cycle_pos" % where
        if info.tax_model == 0:
            assert ((s["tax_rate_idx"] >= 0) & (s["tax_rate_idx"] < len(info.disc))).all()
    if source_list and "regen_src_list" in s:
        hw = info.H * info.W
        want = np.concatenate([np.flatnonzero(wsrc.reshape(-1)), hw + np.flatnonzero(ssrc.reshape(-1))])
        assert int(s["regen_src_n"]) == want.size, "%s: regen_src_n" % where
        cap = s["regen_src_list"].shape[-1]
        got = s["regen_src_list"].astype(np.int16).view(np.uint16)[: min(cap, want.size)]
        assert np.array_equal(got, want[:cap]), "%s: regen_src_list" % where


# ----------------------------------------------------------------------------------------------------------------
# injected states
# ----------------------------------------------------------------------------------------------------------------
STATE_KINDS = ("tax_ladder", "tax_escrow", "book_full_bids", "book_full_asks", "book_ties", "book_resting_asks",
               "book_resting_bids", "crowded", "coin_extremes", "coin_equal", "coin_one", "coin_zero")


def _set_books(s, info, bids, asks):
    """bids / asks: per resource a list of (agent, price, lifetime).  Sorts them as match_orders does and derives the
    counters, histograms and escrows (the coin / resources in escrow come ON TOP of the inventories in `s`)."""
    n, M, P = info.n, info.M, info.P
    s["cda_bids"], s["cda_asks"] = np.zeros((2, M), np.int32), np.zeros((2, M), np.int32)
    s["cda_n_bids"], s["cda_n_asks"] = np.zeros(2, np.int32), np.zeros(2, np.int32)
    s["cda_n_orders"] = np.zeros((2, n), np.int32)
    s["cda_bid_hist"], s["cda_ask_hist"] = np.zeros((2, n, P), np.uint8), np.zeros((2, n, P), np.uint8)
    s["esc_coin"], s["esc_res"] = np.zeros(n), np.zeros((2, n), np.int32)
    for r in range(2):
        bb = sorted(bids[r], key=lambda o: (-o[1], -o[2]))
        aa = sorted(asks[r], key=lambda o: (o[1], -o[2]))
        for k, (ag, pr, life) in enumerate(bb):
            s["cda_bids"][r, k] = ag | (pr << 8) | (life << 16)
            s["cda_bid_hist"][r, ag, pr] += 1
            s["cda_n_orders"][r, ag] += 1
            s["esc_coin"][ag] += pr
        for k, (ag, pr, life) in enumerate(aa):
            s["cda_asks"][r, k] = ag | (pr << 8) | (life << 16)
            s["cda_ask_hist"][r, ag, pr] += 1
            s["cda_n_orders"][r, ag] += 1
            s["esc_res"][r, ag] += 1
        s["cda_n_bids"][r], s["cda_n_asks"][r] = len(bb), len(aa)


def _random_books(info, rng, fill, split=None, expiring=0.15, cap=None):
    """Non-crossing books: every bid at or below `split` - 1, every ask at or above `split` (an agent's own orders may
    cross in the reference, and some do here: asks of an agent below its own bids when nobody else bids that high is
    left out for simplicity), prices bunched so that ties in price and in (price, lifetime) are common."""
    n, P = info.n, info.P
    bids, asks = [[], []], [[], []]
    for r in range(2):
        sp = int(rng.randint(1, P)) if split is None else split
        for i in range(n):
            k = int(round(fill * info.maxo)) if fill >= 1 else int(rng.binomial(info.maxo, fill))
            k = k if cap is None else min(k, cap)
            for _ in range(k):
                life = info.dur if rng.rand() < expiring else int(rng.choice([1, 2, 2, 3, max(1, info.dur - 1)]))
                life = min(max(life, 1), info.dur)
                if rng.rand() < 0.5:
                    bids[r].append((i, int(rng.choice([0, max(sp - 2, 0), sp - 1, sp - 1])), life))
                else:
                    asks[r].append((i, int(rng.choice([sp, sp, min(sp + 1, P - 1), P - 1])), life))
    return bids, asks


def rich_state(env, base, kind, rng, info=None, ordinal=0):
    """An injected state of kind `kind` (STATE_KINDS) for one replica, in the load_state format.  `base`: a state right
    after a reset (every field without the replica dimension): the map, the skills and the generator state are kept,
    the economy is replaced.  `ordinal` counts the replicas of one kind: the tax ladder starts on another cutoff each time."""
    info = info or Info(env)
    n, P = info.n, info.P
    s = {k: np.array(v) for k, v in base.items()}
    # coin: log-uniform over six decades; inventories up to 29; labor of a long episode
    s["inv_coin"] = np.round(10.0 ** rng.uniform(-1, 3.5, size=n), 3)
    s["inv_res"] = rng.randint(0, 30, size=(2, n)).astype(np.int32)
    s["labor"] = np.round(rng.uniform(0, 400, size=n), 2)
    s["timestep"] = np.array(int(rng.randint(1, max(2, info.episode_length - 8))), np.int32)
    bids, asks = [[], []], [[], []]
    if info.has_cda:
        bids, asks = _random_books(info, rng, fill=0.6)
    if info.has_tax:
        s["tax_cycle_pos"] = np.array(info.period, np.int32)  # the first step is a tax day
        s["tax_last_coin"] = np.round(rng.uniform(0, 50, size=n), 3)
        if info.tax_model == 0:
            s["tax_rate_idx"] = rng.randint(0, len(info.disc), size=info.NB).astype(np.int32)
    if kind == "tax_ladder":
        # incomes exactly on every cutoff (in turn), one negative, one inside the effective-rate floor (0, 1e-6), the
        # rest log-uniform over all brackets: coin = income with nothing in escrow and last_coin = 0 keeps the
        # subtraction exact; nobody holds resources or orders, so no coin moves ahead of the levy
        cut = info.cut
        inc = 10.0 ** rng.uniform(-1, np.log10(cut[-1] * 3), size=n)
        on = [0, 1] + list(range(4, n, 2))  # agents 2 and 3 are special, every other one of the rest sits on a cutoff
        for j, i in enumerate(on):
            inc[i] = cut[1 + (2 * ordinal + j) % (info.NB - 1)]
        last = np.zeros(n)
        if n > 2:
            inc[2], last[2] = 2.5, 7.75  # income -5.25
        if n > 3:
            inc[3], last[3] = 2.0 ** -21, 0.0  # 4.8e-7
        s["inv_coin"], s["tax_last_coin"] = inc.copy(), last
        s["inv_res"] = np.zeros((2, n), np.int32)
        bids, asks = [[], []], [[], []]
        if info.tax_model == 0:
            s["tax_rate_idx"] = np.minimum(np.arange(info.NB) * 3 + 2, len(info.disc) - 1).astype(np.int32)
    elif kind == "tax_escrow":
        # high incomes held in escrow: every agent's bid quota full at the maximum price, hardly any coin in hand
        bids = [[(i, P - 1, int(rng.randint(1, info.dur + 1))) for i in range(n) for _ in range(info.maxo)] for _ in range(2)]
        asks = [[], []]
        s["inv_coin"] = np.round(rng.uniform(0, 1.5, size=n), 3)
        s["tax_last_coin"] = np.zeros(n)
        s["inv_res"] = np.zeros((2, n), np.int32)
        if info.tax_model == 0:
            s["tax_rate_idx"] = np.full(info.NB, len(info.disc) - 1, np.int32)
    elif kind in ("book_full_bids", "book_full_asks"):
        # one side of each book holds all M orders, a third of them on their last step; the other side is empty
        hot = rng.rand() < 0.5  # half of these replicas lose orders on the first step, the others keep a full book
        side = [(i, int(rng.choice([2, 3, 3])) if kind == "book_full_bids" else int(rng.choice([6, 6, 7])),
                 info.dur if hot and rng.rand() < 0.34 else int(rng.randint(1, max(2, info.dur))))
                for i in range(n) for _ in range(info.maxo)]
        other = [(i, pr, life) for (i, pr, life) in side]
        rng.shuffle(other)
        if kind == "book_full_bids":
            bids, asks = [side, [(i, pr, life) for i, pr, life in other]], [[], []]
        else:
            bids, asks = [[], []], [side, other]
        s["inv_coin"] = np.round(10.0 ** rng.uniform(0, 2, size=n), 2)
    elif kind in ("book_resting_asks", "book_resting_bids"):
        # every agent one order short of its quota on one side, on one or two prices (the extremes included), and rich
        # enough in coin and resources to take the other side: a step in which everybody does trades n times
        asking = kind == "book_resting_asks"
        for r in range(2):
            prices = [[2, 3, 3], [P - 1], [0]][int(rng.randint(3))]
            side = [(i, int(rng.choice(prices)), int(rng.randint(1, max(2, info.dur - 5)))) for i in range(n)
                    for _ in range(max(1, info.maxo - 1))]
            bids[r], asks[r] = ([], side) if asking else (side, [])
        s["inv_coin"] = np.round(rng.uniform(4 * P, 40 * P, size=n), 2)
        s["inv_res"] = rng.randint(3, 12, size=(2, n)).astype(np.int32)
    elif kind == "book_ties":
        # books one order short of every agent's quota, all bids on two prices and all asks on two prices: coin equal to a
        # price, a single unit of a resource, nothing of the other
        bids, asks = _random_books(info, rng, fill=(info.maxo - 1.0) / info.maxo, split=5, expiring=0.3, cap=info.maxo - 1)
        for r in range(2):  # everybody one short of the quota
            for i in range(n):
                k = sum(o[0] == i for o in bids[r]) + sum(o[0] == i for o in asks[r])
                for _ in range(info.maxo - 1 - k):
                    asks[r].append((i, 5, 2))
        s["inv_coin"] = rng.choice([P - 1.0, P - 1.0, 3.0, 4.0, P - 1.0, 0.0, 250.0], size=n)
        s["inv_res"] = rng.choice([0, 1, 1, 2], size=(2, n)).astype(np.int32)
        s["inv_coin"][3::4], s["inv_res"][:, 3::4] = 4.0, 0  # (the pushy agents of injected_actions: refused for both reasons)
        s["inv_coin"][0] = P - 1.0  # the first bid at the maximum price takes all of agent 0's coin
        if info.has_tax:
            s["tax_cycle_pos"] = np.array(1, np.int32)  # no levy within the run: coin stays equal to a price
    elif kind == "crowded":
        # a built-up map: houses on every free cell around the agents (their own and other agents'), agent 0 walled in
        # by foreign houses / water / the edge, one agent with exactly one Stone and one Wood, inventories past 255
        fl = np.asarray(s["cell_flags"])
        free = (np.asarray(s["stone"]) == 0) & (np.asarray(s["wood"]) == 0) & (fl == 0)
        owner = np.full((info.H, info.W), -1, np.int8)
        occupied = set(zip(s["loc_r"].tolist()[1:], s["loc_c"].tolist()[1:]))
        nbrs = lambda r, c: [(r + dr, c + dc) for dr, dc in ((0, -1), (0, 1), (-1, 0), (1, 0))  # noqa: E731
                             if 0 <= r + dr < info.H and 0 <= c + dc < info.W and not (fl[r + dr, c + dc] & 1)]
        spots = [(r, c) for r in range(info.H) for c in range(info.W)
                 if free[r, c] and (r, c) not in occupied and len(nbrs(r, c)) < 4
                 and all(free[q] and q not in occupied for q in nbrs(r, c))]
        if spots:  # agent 0 moves next to the edge or to water; foreign houses close the rest
            r0, c0 = spots[int(rng.randint(len(spots)))]
            s["loc_r"][0], s["loc_c"][0] = r0, c0
            for q in nbrs(r0, c0):
                owner[q] = 1 + int(rng.randint(n - 1))
        occupied.add((int(s["loc_r"][0]), int(s["loc_c"][0])))
        cand = [(r, c) for r in range(info.H) for c in range(info.W) if free[r, c] and owner[r, c] < 0 and (r, c) not in occupied]
        for k in rng.permutation(len(cand))[: 10 + int(rng.randint(12))]:
            owner[cand[k]] = int(rng.randint(n))
        s["house_owner"] = owner
        s["inv_res"][:, 1 % n] = 1
        s["inv_res"][:, 2 % n] = [256 + int(rng.randint(40)), 300]
        s["labor"] = np.round(rng.uniform(2000, 9000, size=n), 1)
    elif kind == "coin_extremes":
        if info.has_tax:
            s["tax_cycle_pos"] = np.array(1, np.int32)  # no levy (and no lump sum) within the run
        s["inv_coin"] = 10.0 ** rng.uniform(-1, 3, size=n)
        s["inv_coin"][0], s["inv_coin"][n - 1] = 0.0009765625, 131072.5
        bids = [[o for o in bids[r] if o[0] != 0] for r in range(2)]  # nothing of agent 0's in escrow
        s["labor"] = np.round(rng.uniform(3000, 9000, size=n), 1)
    elif kind in ("coin_equal", "coin_one", "coin_zero"):
        bids, asks = [[], []], [[], []]
        s["inv_coin"] = {"coin_equal": np.full(n, 12.5), "coin_one": np.eye(n)[int(rng.randint(n))] * 777.0,
                         "coin_zero": np.zeros(n)}[kind]
        s["inv_res"] = np.zeros((2, n), np.int32)  # nothing to build or sell with: coin stays put
        if info.has_tax:
            s["tax_cycle_pos"] = np.array(1, np.int32)
            s["tax_last_coin"] = s["inv_coin"].copy()
    else:
        raise ValueError(kind)
    if info.has_cda:
        _set_books(s, info, bids, asks)
    s["util"] = np.round(rng.uniform(-50, 50, size=n + 1), 3)
    for k in ("tax_last_income", "tax_last_marginal_rate"):
        if k in s:
            s[k] = np.zeros(n)
    return s



# ----------------------------------------------------------------------------------------------------------------
# scenarios (shared by tests/test_rich_states_cpu.py and tests/test_gpu_rich_states.py)
# ----------------------------------------------------------------------------------------------------------------
LOAD_KEYS = ("stone", "wood", "house_owner", "loc_r", "loc_c", "inv_res", "esc_res", "inv_coin", "esc_coin", "labor", "util",
             "cda_n_bids", "cda_n_asks", "cda_bids", "cda_asks", "cda_n_orders", "cda_bid_hist", "cda_ask_hist",
             "tax_cycle_pos", "tax_rate_idx", "tax_last_coin", "tax_last_income", "tax_last_marginal_rate", "timestep")
INVARIANT_KEYS = LOAD_KEYS + ("cell_flags", "regen_src_n", "regen_src_list")


def scaled_cfg(n_agents=4, episode_length=200, period=50, payment=60, **kw):
    """C2 / C3 with scalars only changed (the compile-time instances still apply): a Build payment and bracket cutoffs
    that put incomes into every bracket, a tax period that fits four levies into a short episode."""
    tax = dict(dict(period=period, usd_scaling=5000.0), **kw.pop("tax", {}))
    cda = dict(dict(order_duration=20), **kw.pop("cda", {}))
    cfg = dict(C2, n_agents=n_agents, episode_length=episode_length, starting_agent_coin=100, resource_regen_prob=0.1,
               env_layout_file="env-pure_and_mixed-25x25.txt",
               components=_components_with(GTB, Build=dict(payment=payment), PeriodicBracketTax=tax, ContinuousDoubleAuction=cda))
    cfg.update(kw)
    return cfg


def _both(*names):
    return tuple("%s[%s]" % (k, r) for k in names for r in ("Stone", "Wood"))


def oracle_env(cfg, E, seed, **env_kw):
    """(host env, OracleEnv) of E replicas, seeded and reset."""
    from helpers import make_env, oracle_host_pre_reset
    from oracle_lib import OracleEnv

    env = make_env(cfg, n_envs=E, **env_kw)
    o = OracleEnv(env.build_config(), env.layout_planes())
    o.seed(seed)
    oracle_host_pre_reset(env, o)
    o.reset()
    return env, o


def rollout_steps(case):
    """One full episode and three steps of the next."""
    return int(case["cfg"]["episode_length"]) + 3


def rollout_on_oracle(case, on_step=None):
    """Runs a ROLLOUTS case on the oracle alone; returns its Reach.  on_step(t, a, p, oracle) sees every step."""
    env, o = oracle_env(case["cfg"], case["E"], case["seed"], **case.get("env_kw", {}))
    info, reach = Info(env), Reach()
    for t in range(rollout_steps(case)):
        a, p = policy_actions(case["policy"], env, o.t["obs_a_action_mask"], o.t["obs_p_action_mask"], case["seed"],
                              int(o.t["timestep"][0]), info)
        before = snapshot(o.t)
        o.step(a, p)
        reach.add(census(before, snapshot(o.t), a, env, info))
        if on_step is not None:
            on_step(t, a, p, o)
        if o.t["done"].all():
            o.reset(o.t["done"].copy())
    assert not o.t["error_flags"].any()
    return reach


def injected_states(case, env, o, info=None):
    """One rich_state per replica (the kinds of the case in turn), built on the oracle's reset states."""
    info = info or Info(env)
    rng = np.random.RandomState(case["seed"])
    states = []
    for e in range(case["E"]):
        base = {k: np.array(o.t[k][e]) for k in INVARIANT_KEYS if k in o.t}
        states.append(rich_state(env, base, case["kinds"][e % len(case["kinds"])], rng, info, ordinal=e // len(case["kinds"])))
    return states


def injected_actions(case, env, o, k, info):
    """Step k of an injected run: NO-OPs first (the masks in the arena are those of the reset; a tax day and the
    expiries happen on untouched coin), then the market script at the steps where everybody bids / everybody asks /
    with every fourth agent of the book states pushy; tax, coin and crowded-map states take the builder's actions."""
    E, n = case["E"], info.n
    if k == 0:
        wp = max(1, len(info.subs_p)) if info.multi_p else 1
        return np.zeros((E, n, len(info.subs) if info.multi else 1), np.int32), np.zeros((E, wp), np.int32)
    # everybody bids for Stone, everybody asks Wood, everybody bids for Wood, everybody asks Stone, a step of resting
    # orders; every other replica of a kind takes the resources the other way round
    kinds = [case["kinds"][e % len(case["kinds"])] for e in range(E)]
    pushy = (np.arange(n)[None, :] % 4 == 3) & np.array([kd.startswith("book") for kd in kinds])[:, None]
    am, pm = o.t["obs_a_action_mask"], o.t["obs_p_action_mask"]
    a = p = None
    for g, seq in enumerate(([12, 34, 32, 14, 1], [32, 14, 12, 34, 1])):
        t = 2 * info.maxo + seq[(k - 1) % 5]
        ag, pg = policy_actions("market", env, am, pm, case["seed"], t, info, pushy=pushy)
        if a is None:
            a, p = ag, pg
        sel = (np.arange(E) // len(case["kinds"])) % 2 == g
        a[sel], p[sel] = ag[sel], pg[sel]
    ab, _ = policy_actions("builder", env, am, pm, case["seed"], 2 * info.maxo + 1, info)
    builders = np.array([kd in ("crowded", "tax_ladder", "coin_equal", "coin_one", "coin_zero") for kd in kinds])
    a[builders] = ab[builders]
    return a, p


def injected_on_oracle(case, on_step=None):
    env, o = oracle_env(case["cfg"], case["E"], case["seed"], **case.get("env_kw", {}))
    info, reach = Info(env), Reach()
    states = injected_states(case, env, o, info)
    for e, s in enumerate(states):
        assert_invariants(s, env, info, "replica %d (%s)" % (e, case["kinds"][e % len(case["kinds"])]))
        o.load_state({k: s[k] for k in LOAD_KEYS if k in s}, e=e)
    for k in range(case["steps"]):
        a, p = injected_actions(case, env, o, k, info)
        before = snapshot(o.t)
        o.step(a, p)
        after = snapshot(o.t)
        reach.add(census(before, after, a, env, info))
        for e in range(case["E"]):  # the reference's invariants hold after every step of the restatement
            assert_invariants({kk: after[kk][e] for kk in INVARIANT_KEYS if kk in after}, env, info, "step %d replica %d" % (k + 1, e))
        if on_step is not None:
            on_step(k, a, p, o)
    assert not o.t["error_flags"].any()
    return reach


_MARKET_REACH = _both("cda_n_trades_in_a_step", "cda_bid_book_full",
                      "cda_equal_price_other_lifetime", "cda_equal_price_equal_lifetime", "cda_buyer_crosses_only_own_asks",
                      "cda_trade_at_ask_price", "cda_trade_at_bid_price", "cda_expiry_in_full_book", "cda_trade_at_price_0",
                      "cda_trade_at_max_price")
_ANNEALED = dict(tax_annealing_schedule=[-1, 0.35])

# name -> policy rollout: E replicas, one episode and the first steps of the next.  kernel: what the device test selects
# and asserts ("instance": the compile-time instance of C2 / C3 -- the changed scalars leave the family; "generic");
# reach: the conditions the rollout must come to (checked on the oracle alone, tests/test_rich_states_cpu.py)
ROLLOUTS = {
    "builder_c2_instance": dict(cfg=scaled_cfg(4), policy="builder", E=64, seed=7, kernel="instance",
                                reach=("build_with_exact_resources", "houses_ge_10", "planner_reward_coin_eq_times_productivity")),
    "market_c2_instance": dict(cfg=scaled_cfg(4), policy="market", E=64, seed=7, kernel="instance",
                               reach=_MARKET_REACH + ("tax_negative_income",)),
    "mix_c3_instance": dict(cfg=scaled_cfg(10), policy="mix", E=64, seed=7, kernel="instance",
                            reach=("tax_every_bracket", "houses_ge_10")
                            + _both("cda_trade_at_ask_price", "cda_trade_at_bid_price")),
    "mix_c2_generic": dict(cfg=scaled_cfg(4, planner_reward_type="inv_income_weighted_utility"), policy="mix", E=64, seed=11,
                           kernel="generic", reach=("houses_ge_10", "planner_reward_inv_income_weighted_utility")
                           + _both("cda_trade_at_ask_price", "cda_trade_at_bid_price")),
    "market_c2_fast_rng": dict(cfg=scaled_cfg(4), policy="market", E=64, seed=13, kernel=None,
                               env_kw=dict(rng_mode="fast"), reach=_both("cda_n_trades_in_a_step", "cda_bid_book_full")),
    "builder_c2_reward_log": dict(cfg=scaled_cfg(4), policy="builder", E=64, seed=17, kernel="instance", reward_log=True,
                                  reach=("houses_ge_10", "build_with_exact_resources")),
    "mix_multi_action_dense_log": dict(
        cfg=scaled_cfg(4, multi_action_mode_agents=True, dense_log_frequency=1, tax=_ANNEALED,
                       planner_reward_type="inv_income_weighted_coin_endowments", mixing_weight_gini_vs_coin=0.3),
        policy="mix", E=64, seed=19, kernel=None,
        reach=_both("cda_bid_and_ask_same_step", "cda_refused_at_quota", "cda_trade_at_ask_price")
        + ("houses_ge_10", "planner_reward_inv_income_weighted_coin_endowments")),
}


def _big_cfg(n, orders, **kw):
    """The 40 x 40 quadrant file with n agents: M = n * orders book slots per side."""
    tax = dict(dict(period=6), **kw.pop("tax", {}))
    cfg = dict(scenario_name="layout_from_file/simple_wood_and_stone", n_agents=n, world_size=[40, 40], episode_length=60,
               starting_agent_coin=60, resource_regen_prob=0.08, env_layout_file="quadrant_40x40_50each.txt",
               components=[["Build", {"payment": 60}], ["ContinuousDoubleAuction", {"max_num_orders": orders, "order_duration": 9}],
                           ["Gather", {}], ["PeriodicBracketTax", tax]])
    cfg.update(kw)
    return cfg


_FIXED11 = dict(tax_model="fixed-bracket-rates", bracket_spacing="linear", n_brackets=11, top_bracket_cutoff=150,
                fixed_bracket_rates=[0.0, 0.05, 0.1, 0.15, 0.22, 0.3, 0.38, 0.45, 0.5, 0.62, 0.8])
_WRAPPER16 = dict(bracket_spacing="linear", n_brackets=16, top_bracket_cutoff=300, rate_disc=0.1,
                  tax_annealing_schedule=[-1, 0.2])
_ALL_KINDS = STATE_KINDS
_BOOK_KINDS = ("book_resting_asks", "book_resting_bids", "book_full_bids", "book_full_asks", "book_ties", "tax_escrow",
               "tax_ladder")
_INJECTED_CDA = _both("cda_n_trades_in_a_step", "cda_bid_book_full", "cda_ask_book_full", "cda_expiry_in_full_book",
                      "cda_trade_at_ask_price", "cda_trade_at_bid_price", "cda_refused_at_quota", "cda_bid_refused_for_coin",
                      "cda_ask_refused_without_inventory", "cda_equal_price_other_lifetime", "cda_equal_price_equal_lifetime")
_INJECTED_TAX = ("tax_every_bracket", "tax_income_on_cutoff", "tax_negative_income", "tax_tiny_income",
                 "tax_due_capped_with_escrow")

# name -> injected run: replica e starts from rich_state(kinds[e % len(kinds)]); `steps` steps (injected_actions)
INJECTED = {
    "wrapper_4ag": dict(cfg=scaled_cfg(4), kinds=_ALL_KINDS, E=48, steps=5, seed=7,
                        reach=_INJECTED_TAX + _INJECTED_CDA + _both("cda_trade_at_price_0", "cda_trade_at_max_price",
                                                                     "cda_bid_accepted_at_coin_equal_price")
                        + ("houses_ge_10", "all_moves_blocked", "inventory_ge_256", "coin_span_1e-3_1e5",
                           "all_agents_equal_coin", "one_agent_holds_all_coin", "total_coin_zero", "all_utilities_negative",
                           "build_with_exact_resources")),
    "us_federal_10ag_multi": dict(
        cfg=scaled_cfg(10, multi_action_mode_agents=True, planner_reward_type="inv_income_weighted_utility",
                       tax=dict(tax_model="us-federal-single-filer-2018-scaled")),
        kinds=_ALL_KINDS, E=36, steps=5, seed=5,
        reach=_INJECTED_TAX + _INJECTED_CDA + ("houses_ge_10", "all_moves_blocked")),
    "annealed_us_federal_wealth_4ag_multi": dict(
        cfg=dict(scaled_cfg(4, multi_action_mode_agents=True, planner_reward_type="inv_income_weighted_coin_endowments",
                            tax=dict(tax_model="us-federal-single-filer-2018-scaled", tax_annealing_schedule=[-1, 0.3]))),
        wealth_ahead_of_tax=True, kinds=_ALL_KINDS, E=36, steps=4, seed=9,
        reach=("tax_annealed_cap_in_high_bracket", "houses_ge_10")),
    "annealed_wrapper_4ag": dict(cfg=scaled_cfg(4, tax=_ANNEALED, multi_action_mode_planner=False), kinds=_ALL_KINDS, E=36,
                                 steps=4, seed=21, reach=_INJECTED_TAX + ("tax_annealed_cap_in_high_bracket",)),
    # M = 64: the largest book a wavefront's registers hold; n trades in a step with 16 agents
    "fixed11_16ag_book64": dict(cfg=_big_cfg(16, 4, tax=_FIXED11), kinds=_BOOK_KINDS, E=21, steps=4, seed=23,
                                reach=("tax_nb_ge8_ragged", "tax_every_bracket", "tax_income_on_cutoff")
                                + _both("cda_n_trades_in_a_step", "cda_bid_book_full", "cda_ask_book_full")),
    # M = 99 > 64: the LDS book
    "fixed11_33ag_book99": dict(cfg=_big_cfg(33, 3, tax=_FIXED11), kinds=_BOOK_KINDS, E=14, steps=4, seed=25,
                                reach=("tax_nb_ge8_ragged", "tax_every_bracket")
                                + _both("cda_n_trades_in_a_step", "cda_bid_book_full", "cda_ask_book_full",
                                        "cda_expiry_in_full_book")),
    # the largest n: 62 trades in one step take more than one order per agent (an agent's bids and asks for a resource share
    # its quota, and the last buyer must not be left with its own ask): M = 186; 16 brackets
    "wrapper16_62ag_book186": dict(cfg=_big_cfg(62, 3, tax=_WRAPPER16), kinds=_BOOK_KINDS, E=14, steps=4, seed=27,
                                   reach=("tax_nb_multiple_of_8", "tax_every_bracket", "tax_annealed_cap_in_high_bracket")
                                   + _both("cda_n_trades_in_a_step", "cda_bid_book_full", "cda_ask_book_full")),
}
for _case in INJECTED.values():
    if _case.pop("wealth_ahead_of_tax", False):
        comps = _case["cfg"]["components"]
        _case["cfg"]["components"] = comps[:3] + [["WealthRedistribution", {}]] + comps[3:]
