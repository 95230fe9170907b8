"""CPU: bench.dump_outputs (--dump-outputs) on host tensors shaped like a tick's outputs: the files
are float64, the sample is the same from call to call, its slices are the tick's own, the totals
cover the whole output and the files stay under the 64 MB bound."""
import os
import types

import numpy as np
import pytest
import torch

import bench


def _tick(M, seed, max_fan):
    rng = np.random.default_rng(seed)
    n = rng.integers(0, max_fan, M)
    offs = np.concatenate([[0], np.cumsum(n)]).astype(np.uint32)
    P = int(offs[-1])
    peers = np.concatenate([rng.integers(0, 1 << 20, P), np.full(1024, 7)]).astype(np.uint32)  # capacity > P
    peers[:3] = [0xFFFFFFFF, 0x80000000, 0]  # u32 ids carried in int32 tensors
    msgs = np.concatenate([np.repeat(np.arange(M), n), np.full(1024, 7)]).astype(np.uint32)
    return n, offs, peers, msgs, P


def _load(d):
    return {f[:-4]: np.load(os.path.join(d, f)) for f in sorted(os.listdir(d))}


# M <= DUMP_ROWS: every row; M > DUMP_ROWS: the seeded sample; fan-out 200: the DUMP_MAX_PAIRS cut
@pytest.mark.parametrize("M,max_fan", [(7, 90), (bench.DUMP_ROWS + 1, 90), (60_000, 200)])
def test_dump_outputs_sample_is_the_ticks_own(tmp_path, M, max_fan):
    n, offs, peers, msgs, P = _tick(M, 1, max_fan)
    t = lambda x: torch.from_numpy(x.view(np.int32))  # noqa: E731
    a = types.SimpleNamespace(dump_outputs=str(tmp_path / "a"))
    bench.dump_outputs(a, 0, 1, t(offs), t(peers), t(msgs), M)
    L = _load(a.dump_outputs)
    assert sorted(L) == ["msgs", "offsets", "peers", "rows", "totals"]
    assert all(v.dtype == np.float64 for v in L.values())
    assert sum(v.nbytes for v in L.values()) <= 64 << 20
    rows = L["rows"].astype(np.int64)
    cut = max_fan == 200  # ~100 pairs a row: DUMP_ROWS rows would hold more than DUMP_MAX_PAIRS
    assert 0 < len(rows) < bench.DUMP_ROWS if cut else len(rows) == min(M, bench.DUMP_ROWS)
    assert (np.diff(rows) > 0).all() and rows[-1] < M
    assert (L["offsets"][:, 0] == offs[rows]).all() and (L["offsets"][:, 1] == offs[rows + 1]).all()
    assert len(L["peers"]) == n[rows].sum() <= bench.DUMP_MAX_PAIRS
    assert (L["peers"] == np.concatenate([peers[offs[m]:offs[m + 1]] for m in rows])).all()
    assert (L["msgs"] == np.repeat(rows, n[rows])).all()
    i64 = lambda x: int(x.astype(np.int64).sum())  # noqa: E731
    assert L["totals"].tolist() == [P, i64(offs), i64(peers[:P]), i64(msgs[:P])]
    # the same call again: the same files; without a message index: no msgs.npy, three totals
    b = types.SimpleNamespace(dump_outputs=str(tmp_path / "b"))
    bench.dump_outputs(b, 1, 2, t(offs), t(peers), None, M)
    L2 = _load(os.path.join(b.dump_outputs, "rank1"))
    assert sorted(L2) == ["offsets", "peers", "rows", "totals"] and len(L2["totals"]) == 3
    assert all(np.array_equal(L[k], L2[k]) for k in ("offsets", "peers", "rows"))
