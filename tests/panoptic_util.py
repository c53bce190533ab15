"""TEST INFRASTRUCTURE — tests/golden/panoptic_device.npz (tools/gen_panoptic_golden.py: id maps and the reference PanopticMetric's
counters on them) as the tests read it."""
import functools
from types import SimpleNamespace

import numpy as np

from util import gold

COUNTERS = ("iou", "true_positive", "false_positive", "false_negative")


@functools.lru_cache(maxsize=None)
def scenes():
    """tag -> namespace(M, updates = [(pred, gt) numpy [B, T, H, W]], ref = {tc: [per update {counter: float32 [2]}]})."""
    G = gold("panoptic_device.npz")
    out = {}
    for tag in (str(t) for t in G["scenes"]):
        n = int(G[f"{tag}.updates"])
        updates = [(G[f"{tag}.u{u}.pred"], G[f"{tag}.u{u}.gt"]) for u in range(n)]
        ref = {tc: [{k: G[f"{tag}.tc{tc}.u{u}.{k}"] for k in COUNTERS} for u in range(n)] for tc in (1, 0)}
        out[tag] = SimpleNamespace(M=int(G[f"{tag}.M"]), updates=updates, ref=ref)
    return out
