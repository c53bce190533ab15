"""CPU: the switch surface is what this file and INTEGRATION.md say it is, and a removed switch no longer moves a plan.

(a) Three sets of SF_* names are read off the sources — the environment variables csrc/ reads (literals passed to geti / getl / isset /
getenv), the ones the Python package reads (os.environ) and the macros csrc/ tests in #if / #ifdef / #ifndef / defined() — and each is
compared with the list below and with the switch table of INTEGRATION.md.  A new switch has to be written down in all three places.

(b) The run-time switches of the conv planners that were removed (their defaults are constants in dispatch.hip / dispatch.h now): a child
process with the variable set plans every case of tests/golden/tiled_plan_parent.json and every row of tests/golden/wino_plan_parent.json
(sf_debug_tiled_plan / sf_debug_wino_plan: host arithmetic, no GPU) and must decide what a child with none of them set decides.  Each
value was chosen so that it DID move a plan at the last commit that read the variable (bb1b5bb) — planned there, on the CPU, with that
commit's library; the first case that moved, of how many:

  SF_DIRECT_CPW=1      tiled affine3x3_64_2x50: ks 4 -> 8                                                              10 cases
  SF_DIRECT_KS=3       tiled affine3x3_64_2x50: ks 4 -> 3                                                              18 cases
  SF_DIRECT_MT=1       tiled affine3x3_64_2x50: mt 2 -> 1                                                               8 cases
  SF_LARGE_P=100000    tiled narrow_1x1_8x50: row 11 (TILE_DMA32x128) -> 12 (TILE_DMA32x32)                            26 cases
  SF_MID_MINCH_LN=8    tiled ln1x1_64_8x50: row 15 (TILE_DMA_SPLIT64x64), 1 K slice -> 13 (TILE_DMA_LN64x128), no split    1 case
  SF_MID_TILES=0       tiled gather_64_1x40: row 4 (TILE_SPLIT64x64), 9 K slices -> 7 (TILE_DMA64x64), no split        10 cases
  SF_SPLIT_CFG=1       tiled gather_64_1x40: row 4 (TILE_SPLIT64x64) -> 1 (TILE_L64x64), 9 K slices kept                8 cases
  SF_SPLIT_FROM=1      tiled affine3x3_64_2x50: row 12 (TILE_DMA32x32) -> 15 (TILE_DMA_SPLIT64x64), 9 K slices          8 cases
  SF_SPLIT_MINCH=8     tiled gather_64_1x40: 9 K slices -> 2                                                            2 cases
  SF_SPLIT_WGS=64      tiled ln7x7_128_2x50: 13 K slices -> 1                                                           8 cases
  SF_SP_MAX_P=0        tiled one_latent_3x3_64: family 2 (small-P) -> 0 (tiled, row 12)                                 6 cases
  SF_WINO_CAT=0        wino split_case_0: form 4 (concatenated), 1408 workgroups -> 2 (plain), 1792                    42 rows
  SF_WINO_CAT_SCALED=0 wino always16_se_scaled_concatenated_stays_32: form 4, 32-tile blocks -> 2, 16-tile blocks       1 row

Removed planner switches for which NO case of the two fixtures moved at bb1b5bb (values tried in brackets), listed and not tested:
SF_SP_BN (32), SF_SP_MAGIC (0), SF_SP_SHORT_TAIL (0), SF_SP_SPLIT_WGS (16), SF_SP_WIDE_WORK (1), SF_SP_XCD (0, 3), SF_WSP_MINSUB (4),
SF_WINO_SP7 (0) — they shape the launch of the small-P kernel, sp_plan, which the two debug entries name as a family and do not describe
—, SF_WINO_GROUP (0: whether run_wino asks wino_plan for a group at all; the entry is always asked with the group) and SF_BF16X3 (0: the
fixtures' split-bf16 layers carry no Winograd weights, and nothing else of a plan depends on it)."""
import json
import os
import re
import subprocess
import sys

import pytest

from util import GOLD, ROOT, tiled_plan, wino_plan

CSRC = os.path.join(ROOT, "streamingflow_amd", "csrc")

# ---- (a) the lists -------------------------------------------------------------------------------------------------------------------
CSRC_ENV = """SF_B3_SMALL_TILES SF_DIRECT SF_DWCONV_PK SF_FLOW_TIMEOUT SF_GLDS SF_HANDOFF_FENCED SF_NARROW SF_PERSIST SF_PIPE
              SF_PLAN_SAMPLE_LAUNCHES SF_PROF_DUMP SF_SMALL_DMA SF_SP SF_SPLIT SF_TRACK_WAVES SF_WIDE64 SF_WINO SF_WINO_CAT_WIDE SF_WINO_LIST
              SF_WINO_LN7 SF_WINO_LN7_MIN_P SF_WINO_MIN_P SF_WINO_SAMPLE SF_WINO_SMALL_WGS SF_WINO_SP SF_WINO_SPLIT_WGS SF_WINO_TALL
              SF_WINO_WHY""".split()
PACKAGE_ENV = "SF_BEVERSE_TORCH SF_LIB_PATH SF_PERSIST SF_PLAN_TORCH SF_SPARSE_SORT SF_TRACK_HOST SF_WINO".split()
CSRC_MACROS = "SF_STAMP SF_STAMP_FLOW".split()


def _sources(top, exts):
    for d, _, files in os.walk(top):
        for f in sorted(files):
            if f.endswith(exts):
                yield open(os.path.join(d, f), encoding="utf-8").read()


def _csrc_env():
    return {m for s in _sources(CSRC, (".hip", ".h")) for m in re.findall(r'\b(?:geti|getl|isset|getenv)\(\s*"(SF_[A-Z0-9_]+)"', s)}


def _package_env():
    pat = r'environ(?:\.get\(|\.pop\(|\.setdefault\(|\[)\s*["\'](SF_[A-Z0-9_]+)["\']|["\'](SF_[A-Z0-9_]+)["\']\s+(?:not\s+)?in\s+\w*\.?environ|getenv\(\s*["\'](SF_[A-Z0-9_]+)["\']'
    return {n for s in _sources(os.path.join(ROOT, "streamingflow_amd"), (".py",)) for m in re.findall(pat, s) for n in m if n}


def _csrc_macros():
    names = set()
    for s in _sources(CSRC, (".hip", ".h")):
        for line in re.findall(r"^[ \t]*#[ \t]*(?:if|ifdef|ifndef|elif)\b(.*)$", s, re.M):
            names |= set(re.findall(r"\bSF_[A-Z0-9_]+\b", line.split("//")[0]))
    return names


def _integration_table():
    """name -> "reader" column of the switch table of INTEGRATION.md (rows `| `SF_X` | default | selects | read by |`)"""
    text = open(os.path.join(ROOT, "INTEGRATION.md"), encoding="utf-8").read()
    rows = re.findall(r"^\| `(-D)?(SF_[A-Z0-9_]+)` \|[^|]*\|[^|]*\|([^|]*)\|$", text, re.M)
    assert len({r[1] + r[0] for r in rows}) == len(rows), "a switch is listed twice"
    return rows


def test_environment_switches_of_csrc_are_the_listed_ones():
    table = {n for d, n, who in _integration_table() if not d and "csrc" in who}
    assert _csrc_env() == set(CSRC_ENV) == table, (_csrc_env() ^ set(CSRC_ENV), set(CSRC_ENV) ^ table)


def test_environment_switches_of_the_package_are_the_listed_ones():
    table = {n for d, n, who in _integration_table() if not d and "package" in who}
    assert _package_env() == set(PACKAGE_ENV) == table, (_package_env() ^ set(PACKAGE_ENV), set(PACKAGE_ENV) ^ table)


def test_compile_time_switches_of_csrc_are_the_listed_ones():
    table = {n for d, n, who in _integration_table() if d}
    assert _csrc_macros() == set(CSRC_MACROS) == table, (_csrc_macros() ^ set(CSRC_MACROS), set(CSRC_MACROS) ^ table)


def test_every_listed_switch_is_in_exactly_one_table_row():
    assert sorted(n for _, n, _ in _integration_table()) == sorted(set(CSRC_ENV) | set(PACKAGE_ENV) | set(CSRC_MACROS))


# ---- (b) removed planner switches ----------------------------------------------------------------------------------------------------
# variable -> the value of the docstring's table
_MOVED = {"SF_DIRECT_CPW": "1", "SF_DIRECT_KS": "3", "SF_DIRECT_MT": "1", "SF_LARGE_P": "100000", "SF_MID_MINCH_LN": "8", "SF_MID_TILES": "0",
          "SF_SPLIT_CFG": "1", "SF_SPLIT_FROM": "1", "SF_SPLIT_MINCH": "8", "SF_SPLIT_WGS": "64", "SF_SP_MAX_P": "0", "SF_WINO_CAT": "0",
          "SF_WINO_CAT_SCALED": "0"}
_NOT_MOVED = "SF_BF16X3 SF_SP_BN SF_SP_MAGIC SF_SP_SHORT_TAIL SF_SP_SPLIT_WGS SF_SP_WIDE_WORK SF_SP_XCD SF_WSP_MINSUB SF_WINO_SP7 SF_WINO_GROUP".split()
_LIVE = ("SF_WINO_SPLIT_WGS", "SF_WINO_CAT_WIDE", "SF_WINO_TALL")      # re-read at every plan: a wino row's own setting is made in the child


def _plans():
    """every case of the two plan fixtures, as {fixture: {case id: plan}}; a Winograd row under its own live switches"""
    tiled = json.load(open(os.path.join(GOLD, "tiled_plan_parent.json")))["cases"]
    wino = json.load(open(os.path.join(GOLD, "wino_plan_parent.json")))["rows"]
    out = {"tiled": {}, "wino": {}}
    for c in tiled:
        out["tiled"][c["id"]] = tiled_plan(c["layers"], c["n"], c["H"], c["W"], epi=c["epi"], flags=c["flags"])
    for r in wino:
        for k in _LIVE:
            os.environ.pop(k, None)
        os.environ.update({k: v for k, v in r.get("env", {}).items() if k in _LIVE})
        out["wino"][r["id"]] = wino_plan(epi=r.get("epi", 0), nprob=r.get("nprob", 1), flags=r.get("flags", 0), **r["layer"])
    return out


@pytest.fixture(scope="module")
def planned():
    """{} and every {variable: value} of _MOVED -> the plans, each setting in a child of its own, all children at once"""
    code = "import json, sys; sys.path.insert(0, %r); import test_switches as t; print(json.dumps(t._plans()))" % os.path.dirname(os.path.abspath(__file__))
    base = {k: v for k, v in os.environ.items() if not k.startswith("SF_") or k == "SF_LIB_PATH"}
    settings = [{}] + [{k: v} for k, v in _MOVED.items()]
    procs = [(s, subprocess.Popen([sys.executable, "-c", code], env=dict(base, **s), stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)) for s in settings]
    res = {}
    for s, p in procs:
        out, err = p.communicate(timeout=300)
        assert p.returncode == 0, (s, err[-2000:])
        res[tuple(s.items())] = json.loads(out.strip().splitlines()[-1])
    return res


def test_nothing_reads_a_removed_planner_switch():
    assert not (set(_MOVED) | set(_NOT_MOVED)) & (_csrc_env() | _package_env())


@pytest.mark.parametrize("name", sorted(_MOVED))
def test_a_removed_switch_moves_no_plan(name, planned):
    unset = planned[()]
    assert len(unset["tiled"]) >= 40 and len(unset["wino"]) >= 40      # the fixtures were planned at all
    assert planned[((name, _MOVED[name]),)] == unset
