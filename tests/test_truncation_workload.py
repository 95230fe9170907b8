"""The workload of tests/test_gpu_truncation.py against the CPU oracle alone: every condition that
keeps the GPU sweep from silently missing a path (block classes, block starts modulo a quad, message
kinds, the radius pass) holds, and the capacity lists are what the sweep expects. Needs no GPU."""
import numpy as np

from test_gpu_truncation import (SLACK, _kinds, alternate, capacities, check_workload, oracle_refs,
                                 short_capacities, workload)


def test_workload_preconditions_and_capacity_lists():
    w = workload()
    refs = oracle_refs(w)
    check_workload(w, refs)
    for ref in (refs.plain, refs.radius):
        kinds = _kinds(w, ref)
        assert len(kinds) == 3
        caps = capacities(ref, kinds)
        short = short_capacities(ref)
        assert set(short) <= set(caps) and caps[0] == 0 and caps[-1] == ref.P + 7 < ref.P + SLACK
        assert {int(g) for g, t in zip(ref.g0, ref.T) if t > 0} <= set(caps)
        order = alternate(caps, ref.P)
        assert set(order) == set(caps)
        kept = [c < ref.P for c in order[:2 * sum(c < ref.P for c in caps)]]
        assert kept[0::2] == [True] * (len(kept) // 2) and kept[1::2] == [False] * (len(kept) // 2)
    assert (refs.plain.msgs == np.repeat(np.arange(w.M), refs.plain.e)).all()
