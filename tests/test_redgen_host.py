"""CPU: the reduce-phase generator (tests/redgen.py) from the oracle alone: every case of tests/test_gpu_reduce_limits.py has the property it is named after -- the
list lengths at mark time (Oracle.export_mark_lengths), the unresolved reads, the connection counts, the hidden buckets -- and the model's counts are the oracle's.
This file is the proof that a case sits on its limit; the GPU module only compares.  No GPU.  Run with -s to see, per case, what was proved."""
import numpy as np
import pytest

import oracle_lib as ol
import redgen as rd


@pytest.fixture(scope="module")
def proved():
    """case, model and the oracle's view of it, made once: status and connections after the initial pass, list lengths and marked entries at mark time, counters"""
    cache = {}

    def get(name):
        if name not in cache:
            c = rd.get_case(name); bases, off = c.arrays()
            o = ol.Oracle(c.k, threads=4); o.add_reads_ascii(bases, off); o.organize(); o.build_index(); o.initial()
            _, _, status, conn = o.export_initial(); status = status.copy()
            o.reduce(); o.convert()
            length, marked = o.export_mark_lengths()
            # (Model with a walk asserts that the construction's counts -- unresolved reads, list lengths, removals, short cut -- are the restatement's)
            cache[name] = dict(case=c, model=c.model(o), status=status, conn=conn, length=length, marked=marked, counters=o.counters(), n_reads=len(off) - 1)
            o.close()
        return cache[name]
    return get


def unresolved_lists(p):
    un = p["status"][1:] == 0
    return sorted(int(x) for x in p["length"][1:][un] if x)


@pytest.mark.parametrize("name", list(rd.CASES))
def test_generator_is_deterministic_per_seed(name):
    a, b = rd.get_case(name), rd.get_case(name)
    (ba, oa), (bb, ob) = a.arrays(), b.arrays()
    assert np.array_equal(ba, bb) and np.array_equal(oa, ob)
    assert len(set(a.reads())) == len(a.reads())                           # no read twice: N is the number of reads
    assert all(len(r) == a.L for r in a.reads())


@pytest.mark.parametrize("name", list(rd.CASES))
def test_model_counts_are_the_oracles(name, proved):
    p = proved(name); m, ctr = p["model"], p["counters"]
    lists = unresolved_lists(p)
    print(f"{name}: N {ctr['N']}, unresolved {m.unresolved}, longest list {m.longest()}, lists > 128 / > 512: {sum(x > 128 for x in lists)} / {sum(x > 512 for x in lists)}, "
          f"removed {m.removed}, hidden buckets {ctr['long_buckets']}, short cut declined {m.declined}, device stats {m.stats('device')}")
    # the restatement's lists are the oracle's, read by read: length at mark time and marked entries
    assert m.walk.length == [int(x) for x in p["length"]] and m.walk.marked == [int(x) for x in p["marked"]]
    assert m.walk.hidden == ctr["long_buckets"]
    assert m.built or name in ("sc_dup", "sc_early", "mixed")             # (the cases with gadgets built by search have no counts from the construction)
    assert ctr["N"] == p["n_reads"]
    assert int((p["status"][1:] == 0).sum()) == m.unresolved
    assert not np.any(p["status"] == 5) and not np.any(p["status"] == 6) and int(p["conn"].max()) <= rd.CONN_LIMIT      # nobody left the unresolved set by the connection limit or by containment
    assert lists == m.lists
    assert not np.any(p["length"][1:][p["status"][1:] != 0])               # only unresolved reads are marked
    assert ctr["transitive_removed"] == int(p["marked"].sum()) == m.removed
    assert (ctr["long_buckets"] > 0) == m.ranked
    assert np.all(p["marked"] <= p["length"])
    for path in ("default", "device", "device_walk", "host"):
        st = m.stats(path)
        assert st["unresolved"] == m.unresolved and st["removed"] == ctr["transitive_removed"]
        assert st["form"] == (3 if path in ("default", "host") else 2 if ctr["long_buckets"] else 1)
        assert None not in st.values()
        if path in ("device", "device_walk"):
            assert st["lists_over_128"] == sum(x > rd.RA_FIRST for x in lists) and st["lists_over_512"] == sum(x > rd.RA_CAP for x in lists)
            assert (st["slices"] == 1) == m.ranked


@pytest.mark.parametrize("name", list(rd.LONGEST))
def test_longest_list_sits_on_the_limit_the_case_is_named_after(name, proved):
    p = proved(name); lists = unresolved_lists(p)
    assert lists[-1] == rd.LONGEST[name] == p["model"].longest()
    if name.startswith("len"):                                             # family A: the marks remove entries of the long list itself
        x = int(np.argmax(p["length"]))
        assert p["marked"][x] > 0 or p["marked"][p["length"] == lists[-1]].sum() > 0
        assert p["model"].removed > 0
    if name.startswith(("ties", "sc_", "nb129")):                          # pure fans: nothing to remove
        assert p["model"].removed == 0 and p["model"].shortcut is not None


@pytest.mark.parametrize("name", list(rd.UNRESOLVED))
def test_unresolved_reads_are_exactly_as_many_as_the_case_says(name, proved):
    p = proved(name)
    assert int((p["status"][1:] == 0).sum()) == rd.UNRESOLVED[name] == p["model"].unresolved
    if name.startswith("few"):
        assert p["counters"]["N"] == rd.UNRESOLVED[name]                  # nothing but the unresolved reads: fewer than the waves of one block
    assert rd.UNRESOLVED["unresolved1024"] == rd.FEW_MAX_THIRD and rd.UNRESOLVED["unresolved1025"] == rd.FEW_MAX_THIRD + 1


def test_empty_and_single_entry_lists(proved):
    for name in ("empty", "single", "few1"):
        p = proved(name); un = p["status"][1:] == 0
        assert np.any(p["length"][1:][un] == 0), name                     # an unresolved read with an empty list
    for name in ("empty", "single", "few2"):
        assert 1 in unresolved_lists(proved(name)) or name == "empty"
    p = proved("empty")
    assert p["counters"]["long_buckets"] > 0 and unresolved_lists(p) in ([1, 1], [1, 1, 1, 1])      # the filler's two chain ends, and the hub with the one B that found it (or nobody)
    assert int((p["length"][1:][p["status"][1:] == 0] == 0).sum()) >= 119                            # the other B: seen by nobody, their hub explored before them


@pytest.mark.parametrize("name", list(rd.POTENTIAL))
def test_potential_list_of_the_blind_hub(name, proved):
    """ranked form: the hub sees no read of the fan (no own hits: its connection count is that of its stem, here none) and every read of the fan sees it, so its
    potential list = the twins = its final list; tests/redgen.py explains why the oracle's serial search then keeps all of them"""
    p = proved(name); m = p["model"]
    assert m.potential[-1] == rd.POTENTIAL[name] == unresolved_lists(p)[-1]
    hub = int(np.argmax(p["length"]))
    assert p["conn"][hub] == 0 and p["counters"]["long_buckets"] > 0
    assert m.stats("device")["potential_over_1024"] == (1 if rd.POTENTIAL[name] > rd.RR_CAP else 0)


def test_short_cut_cases_decline_for_the_reason_they_are_named_after(proved):
    """families C, D, E by the restated short cut (redgen.Walk.shortcut_of): which list it settles, where it gives up and why"""
    def hub(p):
        w = p["model"].walk
        return w, max((r for r in range(1, w.N + 1) if w.unres[r]), key=lambda r: w.length[r])
    for name, n in (("sc_pre7", 7), ("sc_pre8", 8), ("sc_pre9", 9), ("sc_24", 24)):      # a list per entry (every entry is unknown at its turn: also the one beyond the last RA_SC_PRE = 8), settled
        w, h = hub(proved(name))
        assert w.length[h] == n and w.shortcut_of(h) == (n, True, None)
        assert proved(name)["model"].declined.keys() <= {"size"}
    w, h = hub(proved("sc_25"))
    assert w.length[h] == 25 and w.shortcut_of(h) == (rd.RA_SHORTCUT_LISTS + 1, False, "limit") and proved("sc_25")["model"].declined["limit"] == 1
    m = proved("sc_dup")["model"]
    assert m.declined.get("dup", 0) >= 2 and m.removed > 0                 # lists with two entries to one node, and the walk marks entries of them
    assert any(m.walk.marked[r] for r in range(1, m.walk.N + 1) if m.walk.unres[r] and m.walk.shortcut_of(r)[2] == "dup")
    m = proved("sc_early")["model"]
    assert m.declined.get("early", 0) >= 1
    assert any(m.walk.marked[r] for r in range(1, m.walk.N + 1) if m.walk.unres[r] and m.walk.shortcut_of(r)[2] == "early")
    # ... and for some read that test alone decides: without it the short cut would settle the list (a nearer marker is there as the witness)
    alone = [r for r in range(1, m.walk.N + 1) if m.walk.unres[r] and m.walk.shortcut_of(r)[2] == "early" and m.walk.shortcut_of(r, early_rule=False)[1]]
    print("sc_early: the rule alone decides for reads", alone, [(m.walk.length[r], m.walk.marked[r]) for r in alone])
    assert len(alone) >= 3
    for name in ("nb129", "nb513", "ties64", "ties65"):                     # family F: a settled one-entry list whose neighbour's list has that length (64: registers only; 65 and more: the y0 >= 64 loop)
        w, h = hub(proved(name))
        fans = [r for r in range(1, w.N + 1) if w.unres[r] and w.length[r] in (1, 2) and any(e[0] == h for e in w.adj[r])]
        assert len(fans) == w.length[h] == rd.LONGEST[name] and all(w.shortcut_of(r)[1] for r in fans)


def test_mixed_case_holds_every_family(proved):
    p = proved("mixed"); lists = unresolved_lists(p); m = p["model"]
    for n in (1, 2, 9, 24, 25, 65, 129, 256, 513, 1025):
        assert n in lists, n
    assert np.any(p["length"][1:][p["status"][1:] == 0] == 0) and m.ranked and m.removed > 0
    assert {"dup", "early", "limit"} <= m.declined.keys()
    assert sum(m.potential) + m.unresolved > 3 * 1024                     # three slices of 1024 entries and more (SAGE2OV_TEST_RANK_SLICE=1024)
    assert m.unresolved > 5 * 4 * 64                                      # with the marks' grid bound to 3 blocks every wave walks many reads
