"""The torus-world C oracle (oracle/wab_torus_oracle.c) against the golden vectors of the real
Environment 2.0 reference (tests/golden/torus_*.npz, tests/golden/make_golden_torus.py), and
against the reference's own known-answer test (`Environment 2.0/World_tests.py:5-45`)."""
from __future__ import annotations

import json
import os

import numpy as np
import pytest

from oracle.torus_oracle import OracleTorus

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
SETS = ["torus_c3", "torus_multi", "torus_tiny", "torus_continue", "torus_placed"]
# worlds at the edges of what include/wab_torus.h accepts (make_golden_torus.py EDGE_SETS): two
# worlds each, at most 40 turns
EDGE_SETS = ["torus_edge_largest", "torus_edge_line", "torus_edge_unit", "torus_edge_odd5x3",
             "torus_edge_odd9x13", "torus_edge_lone_ostrich", "torus_edge_no_ostriches",
             "torus_edge_no_bushes", "torus_edge_bushes_only", "torus_edge_no_cap", "torus_edge_r128"]


def load_set(name):
    d = np.load(os.path.join(GOLDEN, name + ".npz"))
    meta = json.loads(d["meta"].tobytes())
    return d, meta


def oracle_for(meta, world_id, batch=1, spawn_positions=None):
    return OracleTorus(meta["width"], meta["height"], meta["num_ostriches"], meta["num_wolves"],
                       meta["num_bushes"], meta["options"], batch=batch, seed=meta["seed"],
                       world_id_base=world_id, autoreset=meta["protocol"] == "autoreset",
                       spawn_positions=spawn_positions)


def placed_schedule(d, meta, e):
    """The explicit positions of world index e of a placed set: (create [N, 2] or None,
    {turn: reset positions [N, 2]}; turn 0 is the first reset)."""
    turns = meta.get("placed_resets") or []
    if not turns:
        return None, {}
    return d["create_pos"][e], {t: d["reset_pos"][k, e] for k, t in enumerate(turns)}


@pytest.mark.parametrize("name", SETS + EDGE_SETS)
def test_oracle_reproduces_reference(name):
    d, meta = load_set(name)
    T, NO = meta["T"], meta["num_ostriches"]
    for e, g in enumerate(meta["world_ids"]):
        create, resets = placed_schedule(d, meta, e)
        o = oracle_for(meta, g, spawn_positions=create)
        s = o.state()
        assert np.array_equal(s["df_xy"][0], d["create_df_xy"][e]), "create_* positions"
        o.reset(positions=resets.get(0))
        s = o.state()
        assert np.array_equal(s["obj_xy"][0], d["reset0_obj_xy"][e]), "reset_environment positions"
        for t in range(T):
            if t > 0 and t in resets:
                o.reset(positions=resets[t])
            rec, rew, done, wr = o.step(d["actions"][t, e][None])
            where = "%s world %d turn %d" % (name, g, t)
            bad = np.nonzero((rec[0] != d["records"][t, e]).any(axis=1))[0]
            assert len(bad) == 0, "%s: records of entities %s differ" % (where, bad.tolist())
            assert np.array_equal(rew[0], d["reward"][t, e].astype(np.float32)), where
            assert np.array_equal(done[0].astype(bool), d["done"][t, e]), where
            assert bool(wr[0]) == bool(d["world_reset"][t, e]), where
            s = o.state()
            assert np.array_equal(s["df_xy"][0], d["df_xy"][t, e]), where + " frame X/Y"
            assert np.array_equal(s["obj_xy"][0], d["obj_xy"][t, e]), where + " object x/y"
            assert np.array_equal(s["food"][0], d["food"][t, e]), where + " food"
            assert np.array_equal(s["visible"][0].astype(bool), d["visible"][t, e]), where + " Visible"
            assert np.array_equal(s["status"][0, :NO], d["status"][t, e, :NO]), where + " status"


def wrapped_rows(d, meta):
    """Visible rows whose (Delta_X, Delta_Y) is not the plain difference of the frame positions
    the observer saw (World.py:255-291 replaced it through the wrap), and a check of each: the
    frame X/Y at observation time are df_xy[t] for the entities that acted before the observer
    this turn and the previous turn's (create_df_xy at t = 0) for the others and itself; a reset
    leaves the frame as it was (World.py:355-356).  Every visible row's delta must equal the plain
    one per axis or differ from it by the side (W or H), and be strictly shorter when it does."""
    W, H = meta["width"], meta["height"]
    rec = d["records"]
    T, E, N = rec.shape[:3]
    prev = np.concatenate([d["create_df_xy"][None], d["df_xy"][:-1]], 0).astype(np.int64)
    cur = d["df_xy"].astype(np.int64)
    i_idx = np.arange(N)[:, None]
    j_idx = np.arange(N)[None, :]
    # position of j as observer i saw it: [T, E, i, j, 2]
    pos = np.where((j_idx < i_idx)[None, None, :, :, None], cur[:, :, None, :, :], prev[:, :, None, :, :])
    me = prev[:, :, :, None, :]
    plain = pos - me
    vis = (rec[..., 16:20].copy().view(np.uint32)[..., 0][..., None] >> j_idx.astype(np.uint32)) & 1
    vis = vis.astype(bool)
    dl = rec[..., 24:24 + 2 * N].view(np.int8).astype(np.int64).reshape(T, E, N, N, 2)
    side = np.array([W, H])
    ok_axis = (dl == plain) | ((np.abs(dl - plain) == side) & (np.abs(dl) < np.abs(plain)))
    assert ok_axis.all(-1)[vis].all(), "a visible delta is neither plain nor a shorter wrap"
    return int(((dl != plain).any(-1) & vis).sum())


def visible_rows(d):
    """(visible [T, E, i, j] bool, deltas [T, E, i, j, 2] int64) of a set's records."""
    rec = d["records"]
    N = rec.shape[2]
    j_idx = np.arange(N, dtype=np.uint32)
    vis = ((rec[..., 16:20].copy().view(np.uint32)[..., 0][..., None] >> j_idx) & 1).astype(bool)
    dl = rec[..., 24:24 + 2 * N].view(np.int8).astype(np.int64).reshape(rec.shape[:3] + (N, 2))
    return vis, dl


def early_resets(d, meta):
    """World resets before max_turns turns of an episode: with one ostrich and no ostrich hunger,
    each is a kill (the kill, its loc[j] label quirk and the reset in one turn)."""
    wr = d["world_reset"]
    n = 0
    for e in range(wr.shape[1]):
        ep_len = 0
        for t in range(wr.shape[0]):
            ep_len += 1
            if wr[t, e]:
                n += ep_len < meta["options"]["max_turns"]
                ep_len = 0
    return n


def test_golden_sets_exercise_the_quirks():
    """The fixtures hold what the parity claims rest on: kills, eats, resets, stale frame
    positions after a reset, emptied bushes still eaten, wrapped deltas, x = W spawns."""
    seen = dict(kill=0, eat=0, reset=0, stale=0, wrapped=0, x_eq_w=0, empty_eat=0, label_quirk=0)
    for name in SETS:
        d, meta = load_set(name)
        # every set's view rule is exercised through the wrap, each of its rows checked
        w = wrapped_rows(d, meta)
        assert w >= 500, (name, w)
        seen["wrapped"] += w
    # the benched 1/8/16 set (torus_c3, the wab_torus_kernel<7, 1, 8, 16> instance): kills, each
    # ending its episode early (the hunt worlds, wolves chasing)
    d, meta = load_set("torus_c3")
    assert early_resets(d, meta) >= 20, early_resets(d, meta)
    for name in SETS:
        d, meta = load_set(name)
        W, H, N, NB, NO = meta["width"], meta["height"], d["records"].shape[2], meta["num_bushes"], meta["num_ostriches"]
        seen["reset"] += int(d["world_reset"].sum())
        seen["kill"] += int((np.diff(d["status"][..., :NO].astype(int), axis=0) > 0).sum())
        f = d["food"][..., :NO]
        seen["eat"] += int((np.diff(f, axis=0) > 0).sum())
        seen["x_eq_w"] += int((d["reset0_obj_xy"][..., 0] == W).sum() + (d["obj_xy"][..., 0] == W).sum())
        obj_mod = np.stack([d["obj_xy"][..., 0] % W, d["obj_xy"][..., 1] % H], -1)
        seen["stale"] += int((obj_mod != d["df_xy"]).any(-1).sum())
        bf = d["food"][..., N - NB:]
        seen["empty_eat"] += int((bf == 0).sum())
        vis, st = d["visible"][..., :NO], d["status"][..., :NO]
        seen["label_quirk"] += int(((st == 2) & vis).sum())
    assert seen["kill"] > 20 and seen["eat"] > 50 and seen["reset"] > 20, seen
    assert seen["stale"] > 100 and seen["x_eq_w"] > 0 and seen["empty_eat"] > 0, seen
    assert seen["wrapped"] > 10000, seen
    assert seen["label_quirk"] > 0, seen


def test_edge_sets_hold_what_they_are_for():
    """The edge fixtures, from their arrays alone: every visible row obeys the wrap rule, and
    together the sets hold the cases they were generated for.  (Counts found when the sets were
    generated are in the comments; the floors are well below them.)

    Nothing in Environment 2.0 lowers an ostrich's food, so no ostrich starves (status 1 never
    occurs): the resets of the max_turns = 0 set are all kill-triggered.  The reference's surface
    does allow a bushes-only world (create_ostriches(0), create_wolves(0)):
    torus_edge_bushes_only."""
    wrapped = {}
    for name in EDGE_SETS:
        d, meta = load_set(name)
        wrapped[name] = wrapped_rows(d, meta)  # asserts the per-row rule
        assert d["records"].shape[:2] == (meta["T"], 2) and 20 <= meta["T"] <= 40, name
        assert os.path.getsize(os.path.join(GOLDEN, name + ".npz")) < 150 * 1024, name
    # rows on an odd side whose delta went through the wrap: 311 in 5x3, 1333 in 9x13, 5150 in
    # 127x127, 238 on the line (the unit world, the lone ostrich and the bushes have none)
    assert wrapped["torus_edge_odd5x3"] >= 100 and wrapped["torus_edge_odd9x13"] >= 500, wrapped
    assert wrapped["torus_edge_largest"] >= 2000 and wrapped["torus_edge_line"] >= 100, wrapped
    assert wrapped["torus_edge_unit"] == 0, wrapped
    # a delta of +-63, the longest shorter way round a side of 127: 464 rows in 127x127 (where
    # the 2^20 radius also leaves plain deltas up to 125), 16 on the line (where none is longer)
    for name, floor in (("torus_edge_largest", 100), ("torus_edge_line", 5)):
        d, meta = load_set(name)
        vis, dl = visible_rows(d)
        n63 = {s: int(((dl[..., 0] == s) & vis).sum()) for s in (-63, 63)}
        assert n63[-63] + n63[63] >= floor and min(n63.values()) > 0, (name, n63)
    d, meta = load_set("torus_edge_line")
    vis, dl = visible_rows(d)
    assert np.abs(dl[vis]).max() == 63 and not dl[..., 1].any()
    # resets in every set (4 to 60 each), and N > 1 sets see others than themselves
    for name in EDGE_SETS:
        d, meta = load_set(name)
        assert d["world_reset"].sum() >= 4, name
        vis, _ = visible_rows(d)
        N = vis.shape[2]
        if N > 1:
            assert (vis & ~np.eye(N, dtype=bool)).sum() >= 15, name
    # an eat that takes a bush to 0: one in 127x127 (255 in one eat), 22 and 15 on the odd sides
    emptied = {}
    for name in ("torus_edge_largest", "torus_edge_odd5x3", "torus_edge_odd9x13"):
        d, meta = load_set(name)
        N, NB, NO = d["records"].shape[2], meta["num_bushes"], meta["num_ostriches"]
        bf = d["food"][..., N - NB:]
        before = np.concatenate([np.full_like(bf[:1], meta["options"]["food_per_bush"]), bf[:-1]], 0)
        emptied[name] = int(((bf == 0) & (before > 0)).sum())
        if name == "torus_edge_largest":  # 255 taken at once: an ostrich's food rose by 255
            f = d["food"][..., :NO]
            assert (np.diff(f, axis=0) == 255).any()
    assert emptied["torus_edge_largest"] >= 1 and emptied["torus_edge_odd5x3"] >= 10, emptied
    assert emptied["torus_edge_odd9x13"] >= 5, emptied
    # the line's bushes hold 0 from the start and are rows of the frame all the same
    d, meta = load_set("torus_edge_line")
    assert not d["food"][..., 3:].any() and d["visible"][..., 3:].all()
    # max_turns = 0: no turn cap, so every reset (9, eight of them in the hunt world) follows a
    # turn that left both ostriches killed; and a run of more turns than any cap of the other sets
    d, meta = load_set("torus_edge_no_cap")
    assert meta["options"]["max_turns"] == 0
    wr = d["world_reset"]
    assert wr.sum() >= 5 and wr.any(0).all()
    gaps = np.diff(np.concatenate([[-1], np.nonzero(wr[:, 0])[0], [meta["T"]]]))
    assert gaps.max() > 20, gaps  # world 790 runs its last 36 turns without a reset
    # (the state after a reset turn is the fresh one, so the last kill itself is not in it: the
    # first kills are, status 2 in 56 ostrich-turns, and the episodes' lengths differ as no cap's would)
    assert (d["status"] == 2).sum() >= 20
    assert len(set(np.diff(np.nonzero(wr[:, 1])[0]).tolist())) > 1
    # the sizes the sets are there for
    sizes = {name: load_set(name)[1] for name in EDGE_SETS}
    assert sizes["torus_edge_largest"]["record_size"] == 112 and sizes["torus_edge_r128"]["record_size"] == 128
    assert sizes["torus_edge_lone_ostrich"]["record_size"] == 32 and sizes["torus_edge_unit"]["record_size"] == 32


def test_world_tests_no_wrap_kat():
    """`Environment 2.0/World_tests.py:5-45` (with the options dict World now requires): a
    20x20 world, the ostrich at (10, 10) looking with radius 8 sees all six entities, in id
    order, at these deltas (the reference run gives the same frame)."""
    rows = _visible_rows(20, 20, (10, 10), 8,
                         [(5, 5), (10, 5), (10, 10), (10, 10), (15, 10), (15, 15)])
    assert rows == [(0, -5, -5), (1, 0, -5), (2, 0, 0), (3, 0, 0), (4, 5, 0), (5, 5, 5)]


def test_world_tests_wrap_horizontal_kat():
    """`World_tests.py:49-88`: rows 0-4 as asserted there (Delta_X 6 through the wrap for the
    wolf at x = 5 seen from x = 19).  The test asserts 5 rows; World.py returns 6: the second
    ostrich, moved to (15, 16) by its action 0, is at distance sqrt(52) <= 10 — the test's own
    expectation disagrees with the code (this is what the reference run gives, see the
    `torus_harness` docstring), so the sixth row is checked as the code computes it."""
    rows = _visible_rows(20, 20, (19, 10), 10, [(5, 5), (19, 10), (10, 10), (15, 10), (15, 15), (15, 16)])
    assert rows[:5] == [(0, 6, -5), (1, 0, 0), (2, -9, 0), (3, -4, 0), (4, -4, 5)]
    assert rows[5] == (5, -4, 6)


def _visible_rows(W, H, me, r, xy):
    """World._get_visible_objects' (index, Delta_X, Delta_Y) rows, restated in the oracle's rule
    through a world of len(xy) bushes observed by an ostrich-radius probe."""
    import ctypes

    from oracle.torus_oracle import _lib

    n = len(xy)
    # one ostrich (the observer) + n bushes at the given positions; its radius set to r
    opts = {"gatherer_view_radius": r, "lookout_view_radius": r, "food_per_bush": 20}
    o = OracleTorus(W, H, 1, 0, n, opts, batch=1)
    L = _lib()
    # place the entities: the frame X/Y the rule reads (test hook of the oracle)
    pos = np.array([me] + list(xy), np.int32)
    L.wabt_debug_place.argtypes = [ctypes.c_void_p, ctypes.c_void_p]
    L.wabt_debug_place(o.h, pos.ctypes.data)
    rec = np.zeros(o.R, np.uint8)
    L.wabt_debug_obs.argtypes = [ctypes.c_void_p, ctypes.c_int64, ctypes.c_void_p]
    L.wabt_debug_obs(o.h, 0, rec.ctypes.data)
    vis = int(rec[16:20].view(np.uint32)[0])
    dl = rec[24:24 + 2 * (n + 1)].view(np.int8)
    return [(j - 1, int(dl[2 * j]), int(dl[2 * j + 1])) for j in range(1, n + 1) if vis >> j & 1]
