"""The workload of tests/test_gpu_pair_limit.py against the CPU oracle alone: the ticks' pair counts are
the products the sweep is built on (2^32 - 1, 2^32, two wraps), from the oracle's list lengths; the
closed-form reference equals the oracle's own result wherever the oracle can be asked (the small legal
tick whole, one message of every cube and replication code); and two_wraps' largest capacity lies above
its P modulo 2^32, the case in which a wrapped tick looks complete. Needs no GPU."""
import numpy as np

from test_gpu_pair_limit import (CAP_WRAP, CAPS, CUBE_A, CUBE_B, CUBE_C, CUBE_D, EXCEPT, INCL, LIMIT, N_A, PREFIX,
                                 build_base, check_base, closed_form, light_tick, messages)
from worldql_server_amd import abi


def test_products_closed_form_and_capacities():
    b = build_base()
    check_base(b)
    o = b.oracle
    # the closed form against the oracle: a whole small tick ...
    w, ref = b.ticks["small_legal"], b.refs["small_legal"]
    offs, peers, F = o.route(w.pos, w.world, w.sender, w.repl)
    assert (offs == ref.offs).all() and F == ref.F and ref.P == len(peers) == len(ref.peers)
    assert (peers == ref.peers).all() and (ref.msgs == np.repeat(np.arange(w.M), ref.e.astype(np.int64))).all()
    by_key = o.route(None, w.world, w.sender, w.repl, keys=w.keys)
    assert (by_key[0] == offs).all() and (by_key[1] == peers).all()
    # ... and single messages: every cube, IncludingSelf / ExceptSelf / an unknown code, senders at the
    # list's ends, inside it and outside it
    for c in (CUBE_A, CUBE_B, CUBE_C, CUBE_D):
        for rp in (INCL, EXCEPT, 7):
            for s in (0, 7, 4099, 65535, 65536, 69999):
                m = messages([c], [rp])
                m.sender[:] = s
                offs, peers, F = o.route(m.pos, m.world, m.sender, m.repl)
                ref = closed_form(m.cube, b.lists, m.sender, m.repl, 1 << 20)
                assert (offs == ref.offs).all() and (peers == ref.peers).all() and F == ref.F, (c, rp, s)
    g = b.ticks["global_legal"]
    offs, peers = o.route_global(g.world[:3], g.sender[:3], g.repl[:3])
    assert (offs == b.refs["global_legal"].offs[:4]).all() and (peers[:PREFIX] == b.refs["global_legal"].peers).all()
    # the legal ticks' last offset fits u32 exactly; the over-limit ones' does not
    for name, ref in b.refs.items():
        assert (ref.P <= LIMIT) == (int(ref.offs[-1]) == ref.P)
    # capacities: never sized for P, and two_wraps' largest one above its wrapped P
    assert max(CAPS) < PREFIX and b.refs["two_wraps"].P % (1 << 32) < CAP_WRAP < LIMIT
    assert abi.MAX_PAIRS == LIMIT and N_A * 65535 == LIMIT


def test_tag_wrap_ticks():
    """The tag-wrap test's two long ticks have 4,096 blocks each and different block totals."""
    b = build_base()
    totals = {}
    for kind in ("even", "blocks"):
        w = light_tick(kind)
        offs, _, _ = b.oracle.route(w.pos, w.world, w.sender, w.repl)
        assert w.M == 4096 * 256
        totals[kind] = np.diff(offs[0::256].astype(np.int64))
    assert len(set(totals["even"].tolist())) == 1 and len(set(totals["blocks"].tolist())) >= 3
    assert light_tick("one").M <= 256
