"""CPU: the host half of the short-interval instance tracking (streamingflow_amd.instance._consistent_tables) against the
REFERENCE's results (tests/golden/instance_short_interval.npz, tools/gen_instance_seq_golden.py: streamingflow/utils/instance.py
as is).  The per-frame maps the fixture stores stand in for the device half; their counts and centres are taken with the
arithmetic of instance_moments (integer sums / count in float64, then float32).  Ids must match exactly."""
import os
import sys

import numpy as np
import pytest

from util import ROOT, gold

sys.path.insert(0, os.path.join(ROOT, "tools"))
import gen_instance_seq_golden as GEN  # noqa: E402

CAP = 100


def moments(frames):
    """frames [T, H, W] -> (counts [T, K] int32, centres [T, K, 2] float32), K = CAP + 1, id 0 not counted."""
    T, H, W = frames.shape
    counts = np.zeros((T, CAP + 1), dtype=np.int32)
    sums = np.zeros((T, CAP + 1, 2), dtype=np.int64)
    rows, cols = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    for t in range(T):
        ids = frames[t].astype(np.int64)
        on = ids > 0
        np.add.at(counts[t], ids[on], 1)
        np.add.at(sums[t, :, 0], ids[on], rows[on])
        np.add.at(sums[t, :, 1], ids[on], cols[on])
    with np.errstate(invalid="ignore", divide="ignore"):
        centres = (sums / counts[..., None].astype(np.float64)).astype(np.float32)
    return counts, centres


@pytest.mark.parametrize("tag", sorted(GEN.SCENES))
def test_short_interval_tables_reproduce_the_reference(tag):
    from streamingflow_amd import instance as I
    G = gold("instance_short_interval.npz")
    raw, want = G[f"{tag}.raw"].astype(np.int64), G[f"{tag}.short"].astype(np.int64)
    assert raw.shape == want.shape == (GEN.SCENES[tag][2], GEN.SCENES[tag][3], GEN.H, GEN.W)
    for b in range(raw.shape[0]):
        counts, centres = moments(raw[b])
        tables = I._consistent_tables(counts, centres, centres, 10.0)
        assert tables.shape == (raw.shape[1], CAP + 1) and tables.dtype == np.int64
        got = np.take_along_axis(tables, raw[b].reshape(raw.shape[1], -1), axis=1).reshape(raw[b].shape)
        assert np.array_equal(got, want[b]), (tag, b)


def test_fixture_tells_the_two_matchers_apart():
    G = gold("instance_short_interval.npz")
    assert np.array_equal(G["s0k1.short"], G["s0k1.regular"])            # consecutive frames: they agree
    for tag in ("s1k4", "s3k6"):
        assert not np.array_equal(G[f"{tag}.short"], G[f"{tag}.regular"]), tag
    assert int(G["s1k4.short"].max()) == 5 and int(G["s1k4.regular"].max()) == 9
    assert int(G["s3k6.short"].max()) == 10 and int(G["s3k6.regular"].max()) == 15      # matches beyond 10 pixels start new ids
    assert G["s2k4e.short"].max(axis=(2, 3)).tolist() == [[5, 5, 0, 4, 4]]              # after the empty frame: raw ids again
