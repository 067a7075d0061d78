"""GPU: the hub form of step 5's solver (k_mf_hub_*; sage2ov_mcf_hub_stats_get): lists longer than the threshold are walked by a workgroup per
tile of their entries.  The form changes who walks a list and no number: every network here is held against tests/flow_model.py exactly -- flows, prices, phases,
rounds, pushes, relabels and price updates -- with the threshold lowered to 300 (SAGE2OV_TEST_MCF_HUB_DEG) so that lists of a few hundred to 20 001 entries are hubs,
and the hub form's own counters say that it, and not the node's workgroup, did the work.  The tile size is read from the library: the degrees follow it."""
import numpy as np
import pytest

import flow_model as fm
import flowgen as fg
import sage2_amd as s2
from test_gpu_copycount import golden_ctx
from test_gpu_flow import ERR_ARG, ERR_LIMIT, OPTIMA, network_cost_and_certificate

pytestmark = [pytest.mark.gpu, pytest.mark.usefixtures("minimiser_groups_on")]
HUB, LDS = "SAGE2OV_TEST_MCF_HUB_DEG", "SAGE2OV_TEST_MCF_LDS"
COUNTERS = ("phases", "rounds", "pushes", "relabels", "price_updates")
FEW = {301: 100, 2049: 700, 6161: 2000, 20001: 7000}                                   # forced units of the "few" shapes (about a third of the degree)


@pytest.fixture(scope="module")
def ctx():
    c = s2.Context(21)
    yield c
    c.close()


@pytest.fixture
def env(monkeypatch, ctx):
    """env(hub=..., lds=...): the two test variables (None: unset) as the context reads them; both unset again afterwards"""
    def put(hub="300", lds="0"):
        for k, v in ((HUB, hub), (LDS, lds)):
            if v is None: monkeypatch.delenv(k, raising=False)
            else: monkeypatch.setenv(k, v)
        ctx.options_reload()
    yield put
    monkeypatch.delenv(HUB, raising=False); monkeypatch.delenv(LDS, raising=False); ctx.options_reload()


@pytest.fixture(scope="module")
def tile(ctx):
    n, arcs = fg.hand("one_path"); ctx.mcf_solve(n, arcs)
    t = ctx.mcf_hub_stats()["tile"]
    assert t >= 256 and t % 256 == 0
    return t


_models = {}


def model(key, n, arcs, **kw):
    if key not in _models: _models[key] = fm.solve(n, *fg.split(arcs), **kw)
    return _models[key]


def counters(st):
    return tuple(int(getattr(st, c)) for c in COUNTERS)


def exact(ctx, key, n, arcs, wide=False):
    """one solve held against the model and the certificate; returns (flow, prices as Python integers, counters, hub statistics)"""
    r = model(key, n, arcs)
    assert r.status == fm.OK
    flow, price, st = ctx.mcf_solve(n, arcs, wide=wide)
    hs = ctx.mcf_hub_stats()
    print(f"{key}: n {n} arcs {len(arcs)} wide {wide} counters {counters(st)} hub {hs} solve {st.solve_ms:.2f} ms")
    assert st.form == s2.MCF_FORM_LAUNCHES and st.price_words == (2 if wide else 1)
    price = [int(x) for x in price]
    assert np.array_equal(flow, r.flow) and price == [int(x) for x in r.price]
    assert counters(st) == (r.phases, r.rounds, r.pushes, r.relabels, r.updates)
    assert fm.certificate(n, *fg.split(arcs), flow, np.array(price, np.int64), st.scale) == r.total_cost == st.total_cost
    return flow, price, counters(st), hs


def degree_of(name, tile):
    return {"300": 300, "301": 301, "T": tile, "T+1": tile + 1, "3T+17": 3 * tile + 17, "20001": 20001}[name]


def shape(name, kind, tile):
    d = degree_of(name, tile)
    return d, fg.hub(d, FEW.get(d, d // 3) if kind == "few" else d - 1)


def check_hub_counters(hs, d, kind, tile):
    if d <= 300:
        assert (hs["hub_deg"], hs["hubs"], hs["tiles"], hs["hub_pushes"], hs["hub_relabels"]) == (300, 0, 0, 0, 0)
        return
    assert (hs["hub_deg"], hs["tile"], hs["hubs"], hs["tiles"]) == (300, tile, 2, 2 * ((d + tile - 1) // tile)) and hs["hub_pushes"] > 0
    if kind == "few": assert hs["hub_relabels"] > 0                                    # (the "all" shapes relabel a hub once and never clip: the pushes only)


# ------------------------------------------------------------------------------------------ 1, 5: both sides of every threshold, both widths
DEGREES = ["300", "301", "T", "T+1", "3T+17", "20001"]


@pytest.mark.parametrize("kind", ["few", "all"])
@pytest.mark.parametrize("name", DEGREES)
def test_hubs_on_both_sides_of_every_threshold(ctx, env, tile, name, kind):
    d, (n, arcs) = shape(name, kind, tile)
    deg = np.bincount(np.concatenate([arcs["from"], arcs["to"]]).astype(np.int64), minlength=n + 1)
    assert deg[1] == d and deg[2] == d and deg[3:].max() == 2
    env()
    _, _, _, hs = exact(ctx, f"hub_{d}_{kind}", n, arcs)
    check_hub_counters(hs, d, kind, tile)


@pytest.mark.parametrize("kind", ["few", "all"])
@pytest.mark.parametrize("name", DEGREES)
def test_hubs_with_128_bit_prices_word_for_word(ctx, env, tile, name, kind):
    d, (n, arcs) = shape(name, kind, tile)
    env()
    narrow = exact(ctx, f"hub_{d}_{kind}", n, arcs)
    wide = exact(ctx, f"hub_{d}_{kind}", n, arcs, wide=True)
    assert np.array_equal(narrow[0], wide[0]) and narrow[1:3] == wide[1:3]
    check_hub_counters(wide[3], d, kind, tile)
    assert {k: v for k, v in wide[3].items()} == {k: v for k, v in narrow[3].items()}


# ------------------------------------------------------------------------------------------ 2: the clip beyond the first tile
def hub_cheap_last(degree, forced):
    """fg.hub with the hub's arcs by cost descending: the cheap entries -- the admissible ones -- are the last of node 1's list, so the excess ends in a late tile"""
    n, a = fg.hub(degree, forced); d = degree - 1
    a["cost"][1:1 + d] = np.sort(a["cost"][1:1 + d])[::-1]
    return n, a


@pytest.mark.parametrize("wide", [False, True])
@pytest.mark.parametrize("degree, forced, rounds", [(6161, 2000, 173), (20001, 7000, 94)])
def test_the_clip_beyond_the_first_tile(ctx, env, tile, degree, forced, rounds, wide):
    n, arcs = hub_cheap_last(degree, forced)
    first = arcs["cost"][1:degree]
    assert np.all(first[:-1] >= first[1:]) and degree > 2 * tile
    assert model(f"cheap_last_{degree}", n, arcs).rounds == rounds                     # (70 and 10 of them clip a hub in a tile behind its first)
    env()
    _, _, _, hs = exact(ctx, f"cheap_last_{degree}", n, arcs, wide=wide)
    assert (hs["hubs"], hs["tiles"]) == (2, 2 * ((degree + tile - 1) // tile)) and hs["hub_pushes"] > 0 and hs["hub_relabels"] > 0


# ------------------------------------------------------------------------------------------ 3: hubs away from workgroup 0 and apart from each other
def test_hubs_anywhere_in_the_node_numbers(ctx, env, tile):
    n, arcs = fg.hub(6161, 2000)
    perm = np.random.default_rng(77).permutation(n).astype(np.uint32) + 1              # node v becomes perm[v - 1]
    arcs = arcs.copy(); arcs["from"] = perm[arcs["from"] - 1]; arcs["to"] = perm[arcs["to"] - 1]
    a, b = int(perm[0]), int(perm[1])
    assert (a - 1) // 256 != 0 and (b - 1) // 256 != 0 and (a - 1) // 256 != (b - 1) // 256      # neither in workgroup 0, not in one workgroup
    env()
    _, _, _, hs = exact(ctx, "hub_6161_permuted", n, arcs)
    assert (hs["hubs"], hs["tiles"]) == (2, 2 * ((6161 + tile - 1) // tile)) and hs["hub_pushes"] > 0 and hs["hub_relabels"] > 0


# ------------------------------------------------------------------------------------------ 4, 6: the real shape; on, off, default
def test_the_real_shape_against_the_model(ctx, env, tile):
    n, arcs = fg.generated("shape_s3")
    deg = np.bincount(np.concatenate([arcs["from"], arcs["to"]]).astype(np.int64), minlength=n + 1)
    assert deg[1] == 801 and deg[2] == 801 and deg[3:].max() <= 24
    env()
    _, _, _, hs = exact(ctx, "shape_s3", n, arcs)
    assert (hs["hubs"], hs["tiles"]) == (2, 2 * ((801 + tile - 1) // tile)) and hs["hub_pushes"] > 0 and hs["hub_relabels"] > 0


@pytest.mark.parametrize("name", ["ring_600", "shape_s3"])
def test_on_off_and_default_give_the_same_numbers(ctx, env, name):
    n, arcs = fg.generated(name)
    deg = np.bincount(np.concatenate([arcs["from"], arcs["to"]]).astype(np.int64), minlength=n + 1)[1:]
    got = {}
    for setting in ("0", "300", None):
        env(hub=setting, lds=None)
        got[setting] = exact(ctx, name, n, arcs)
        hs = got[setting][3]
        want_deg = {"0": 0, "300": 300, None: s2.MCF_HUB_DEG}[setting]
        assert hs["hub_deg"] == want_deg and hs["hubs"] == (int((deg > want_deg).sum()) if want_deg else 0)
    assert got["0"][3]["hub_pushes"] == 0 and got[None][3]["hubs"] == 0
    assert got["300"][3]["hubs"] == (2 if name == "shape_s3" else 0)
    for setting in ("300", None):
        assert np.array_equal(got["0"][0], got[setting][0]) and got["0"][1:3] == got[setting][1:3]


# ------------------------------------------------------------------------------------------ 7: infeasible at a hub
def test_infeasible_at_a_hub(ctx, env):
    n, arcs = fg.hub(301, 100); arcs = arcs.copy(); arcs[0]["lower"] = 400; arcs[0]["upper"] = 400
    r = model("hub_301_infeasible", n, arcs)
    assert (r.status, r.rounds) == (fm.INFEASIBLE, 2)
    env()
    for wide in (False, True):
        with pytest.raises(s2.Sage2ovError) as e: ctx.mcf_solve(n, arcs, wide=wide)
        assert e.value.code == ERR_ARG and "infeasible" in str(e.value)
        assert ctx.mcf_hub_stats()["hubs"] == 2
    n, arcs = fg.hub(301, 100)
    exact(ctx, "hub_301_few", n, arcs)


# ------------------------------------------------------------------------------------------ 8: the round budget
def test_round_budget_with_hubs(ctx, env):
    n, arcs = fg.hub(20001, 7000)
    r = model("hub_20001_few_20_rounds", n, arcs, max_rounds=20)
    assert r.status == fm.LIMIT
    stats = {}
    for setting in ("300", "0"):
        env(hub=setting)
        with pytest.raises(s2.Sage2ovError) as e: ctx.mcf_solve(n, arcs, max_rounds=20)
        assert e.value.code == ERR_LIMIT
        st = ctx.mcf_stats(); stats[setting] = counters(st) + (int(st.nodes), int(st.arcs))
        assert (st.rounds, st.pushes, st.relabels) == (20, r.pushes, r.relabels)
        hs = ctx.mcf_hub_stats()
        assert hs["hubs"] == (2 if setting == "300" else 0) and (hs["hub_pushes"] > 0) == (setting == "300")
    assert stats["300"] == stats["0"]


# ------------------------------------------------------------------------------------------ 9: the resident route
def test_the_resident_network_with_hubs(monkeypatch, tmp_path):
    name = "g13_noisy300_k55"; flows = {}
    for setting in ("300", "0"):
        monkeypatch.setenv(HUB, setting)
        c = golden_ctx(name, tmp_path)
        c.genome_size(); c.flow_network_build(); st = c.flow_solve()
        assert network_cost_and_certificate(c) == OPTIMA[name] == 19999938 == st.total_cost
        hs = c.mcf_hub_stats()
        assert (hs["hub_deg"], hs["hubs"]) == ((300, 2) if setting == "300" else (0, 0)) and (hs["hub_pushes"] > 0) == (setting == "300")
        flows[setting] = (c.flow_solution()[0], c.flow_solution()[1], counters(st))
        c.close()
    monkeypatch.delenv(HUB)
    assert np.array_equal(flows["300"][0], flows["0"][0]) and np.array_equal(flows["300"][1], flows["0"][1]) and flows["300"][2] == flows["0"][2]
