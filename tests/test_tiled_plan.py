"""CPU: the plan of the tiled conv kernels (dispatch.hip: tiled_plan, asked through sf_debug_tiled_plan — host arithmetic, no GPU) is the
parent commit's.  tests/golden/tiled_plan_parent.json holds, per case and switch setting, what the commit named in it decided: its five plan
integers (cfg, mt, ks, glds_tile, glds_var), the K slices per problem, the profiler key and the kernel instantiation those integers selected
in its launcher (the fixture says how they were recorded), and the mapping from those integers to the rows of the tile table
(csrc/sf_launch.h: TILES) that replaced them.  The cases: the smallest layer that reaches each outcome — every table row, each with and
without split-K scratch, a gathered layer, a narrow one, SE-scaled AFFINE and SAMPLE layers, a GRU candidate with the reset gate applied
while staging, groups of two problems of different cout_pad, a LayerNorm layer over 65..128 channels, a 7x7 at mid P that splits — under
the defaults and under nine switch settings, and under SF_NARROW = 4 / 6 / 7 / 10, whose value names the tile of a narrow layer.  The
switches are read once per process: every setting is planned by a child process.

What this does NOT test: the launcher.  'instantiation' is compared with what the debug entry says the table row stands for (its "row that
runs" and the fixture's shape of that row, which test_fixture_rows_are_the_table holds to the TILES columns) — not with what
launch_conv_glds / launch_conv launch.  That (row, epilogue, scale) -> kernel mapping is covered on the GPU: the kernel-name tests of
test_gpu_ops.py / test_gpu_conv_random.py / test_gpu_sparse_conv.py / test_gpu_bf16x3.py, and the recorded kernel traces and device-code
comparison under profiles/ (refactor_tiled_table_*)."""
import json
import os
import re
import subprocess
import sys

import pytest

from util import GOLD, ROOT, tiled_plan

_FIX = json.load(open(os.path.join(GOLD, "tiled_plan_parent.json")))
_CASES = _FIX["cases"]
_ROWS = [r["name"] for r in _FIX["rows"]]


def _plans():
    return [tiled_plan(c["layers"], c["n"], c["H"], c["W"], epi=c["epi"], flags=c["flags"]) for c in _CASES]


def _row_of(p):
    """the table row the parent's integers stand for, by the fixture's mapping"""
    m = _FIX["mapping"]["cfg"][str(p["cfg"])] if p["glds_tile"] < 0 else _FIX["mapping"]["glds_tile"][str(p["glds_tile"])]
    return m if isinstance(m, str) else m["glds_var"][str(p["glds_var"])]


def _instantiation(case, plan):
    """the instantiation the row that runs stands for, in the fixture's notation"""
    r, en = _FIX["rows"][plan["runs"]], _FIX["epilogues"][case["epi"]]
    if r["kernel"] == "conv_direct_kernel":
        return "conv_direct_kernel<%d,%s> ks=%d" % (plan["mt"], en, plan["ks"])
    scale = r["kernel"] == "conv_glds_kernel" and (case["epi"] == 4 or case["flags"] & 4)
    return "%s<%s,%s%s>" % (r["kernel"], r["shape"], en, ",SCALE" if scale else "")


@pytest.fixture(scope="module")
def planned():
    """env (as a sorted tuple) -> the plans of every case, each setting in a child of its own, all children at once"""
    code = ("import json, sys; sys.path.insert(0, %r); import test_tiled_plan as t; print(json.dumps(t._plans()))" % os.path.dirname(os.path.abspath(__file__)))
    base = {k: v for k, v in os.environ.items() if not k.startswith("SF_") or k == "SF_LIB_PATH"}
    procs = [(s["env"], subprocess.Popen([sys.executable, "-c", code], env=dict(base, **s["env"]), stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True))
             for s in _FIX["parent"]]
    res = {}
    for env, p in procs:
        out, err = p.communicate(timeout=300)
        assert p.returncode == 0, (env, err[-2000:])
        res[tuple(sorted(env.items()))] = json.loads(out.strip().splitlines()[-1])
    return res


def test_fixture_names_its_source():
    assert re.fullmatch(r"[0-9a-f]{40}", _FIX["source"]["commit"])
    assert {s["origin"] for s in _FIX["parent"]} <= {"hooked", "traced"} and "not committed" in _FIX["source"]["how"]
    assert len({c["id"] for c in _CASES}) == len(_CASES) and all(len(s["plans"]) == len(_CASES) for s in _FIX["parent"])
    assert [s["env"] for s in _FIX["parent"]] == [{}, {"SF_GLDS": "0"}, {"SF_SMALL_DMA": "-1"}, {"SF_DIRECT": "0"}, {"SF_SPLIT": "0"}, {"SF_WIDE64": "1"},
                                                   {"SF_NARROW": "-1"}, {"SF_B3_SMALL_TILES": "1"}, {"SF_SP": "0"}, {"SF_WINO": "0"},
                                                   {"SF_NARROW": "4"}, {"SF_NARROW": "6"}, {"SF_NARROW": "7"}, {"SF_NARROW": "10"}]
    # every case comes with and without the split-K scratch (flag 16)
    assert {c["id"] for c in _CASES if not c["flags"] & 16} == {c["id"] + "_noscratch" for c in _CASES if c["flags"] & 16}


def test_fixture_rows_are_the_table():
    """the fixture's rows are enum TileId of sf_launch.h, in order, with the kernel and MT,NT,WM,WN[,KS] of the TILES columns, and every one of
    them is hit by at least one case"""
    src = open(os.path.join(ROOT, "streamingflow_amd", "csrc", "sf_launch.h")).read()
    enum = re.search(r"enum TileId \{(.*?)TILE_COUNT", src, re.S).group(1)
    assert [n.strip() for n in enum.split(",") if n.strip()] == _ROWS
    table = {m.group(1): (m.group(2), [int(v) for v in m.group(3).split(",")])
             for m in re.finditer(r"/\* (TILE_\w+) +\*/ \{(TILE_\w+), (\d+, \d+, \d+, \d+, \d+),", src)}
    for r in _FIX["rows"]:
        staging, dims = table[r["name"]]
        want = {"TILE_STAGED": ("conv_igemm_kernel", ",".join(map(str, dims))), "TILE_DMA": ("conv_glds_kernel", ",".join(map(str, dims[:4]))),
                "TILE_DIRECT": ("conv_direct_kernel", "mt")}[staging]
        assert (r["kernel"], r["shape"]) == want, r
    hit = {_row_of(p) for s in _FIX["parent"] for p in s["plans"] if p["family"] == 0}
    assert hit == set(_ROWS), set(_ROWS) - hit


@pytest.mark.parametrize("setting", _FIX["parent"], ids=lambda s: ",".join("%s=%s" % kv for kv in s["env"].items()) or "defaults")
def test_plan_is_the_parents(setting, planned):
    plans = planned[tuple(sorted(setting["env"].items()))]
    assert len(plans) == len(_CASES)
    for case, was, now in zip(_CASES, setting["plans"], plans):
        what = (case["id"], setting["env"], was, now)
        assert now["family"] == was["family"], what
        if was["family"]:      # the Winograd / small-P kernel's: the tiled planner is not asked
            continue
        assert _ROWS[now["row"]] == _row_of(was), what
        assert (now["mt"], now["ks"], now["nsplit"], now["key"]) == (was["mt"], was["ks"], was["nsplit"], was["key"]), what
        assert _instantiation(case, now) == was["instantiation"], what


def test_narrow_value_that_names_no_tile_fails():
    """SF_NARROW=5 is no variant number: the parent's launcher answered hipErrorInvalidValue for such a narrow layer (SF_ERR_LAUNCH, -3, from the
    dispatch); the plan says so now.  A layer that is not narrow is planned as ever"""
    code = ("import sys; sys.path.insert(0, %r); from util import tiled_plan\n"
            "print(tiled_plan([dict(c0=64, c1=0, cout=64, k=1)], 8, 50, 50)['row'])\n"
            "try:\n    tiled_plan([dict(c0=64, c1=0, cout=32, k=1)], 8, 50, 50)\n    print('planned')\n"
            "except RuntimeError as e:\n    print('refused' if '(-3)' in str(e) else e)\n" % os.path.dirname(os.path.abspath(__file__)))
    env = {k: v for k, v in os.environ.items() if not k.startswith("SF_") or k == "SF_LIB_PATH"}
    r = subprocess.run([sys.executable, "-c", code], env=dict(env, SF_NARROW="5"), capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    assert r.stdout.split() == [str(_ROWS.index("TILE_DMA64x64")), "refused"], r.stdout
