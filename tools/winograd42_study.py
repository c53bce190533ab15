"""Accuracy study for the tall-tile Winograd form F(4,3) along y x F(2,3) along x (conv_wino.hip, TALL) — CPU, test infrastructure only.

Every non-dilated 3x3 / stride-1 convolution of the oracle (oracle/ref_torch.py; ConvTranspose2d(k3, s1, p1) as the equivalent
convolution) — the layers that take a 32-tile launch of the Winograd kernel in the batched forward — is re-evaluated as
    U = G4 g G2^T (6x4 per cout, cin),  V = B4^T d B2 (per 6x4 input tile, stride 4 x 2),  M = sum_cin U (.) V,  Y = A4^T M A2 (4x2 outputs)
in fp32 with Lavin's F(4,3) and F(2,3) matrices: 12 multiplies per 2x2 outputs and (cin, cout) pair instead of 16.  Everything else as
shipped: the dilated ASPP branches through their polyphase components in F(2x2, 3x3) (tools/r04/winograd_study.py), all other layers in
the direct form.  The oracle runs one sample, so the study switches a superset of what any batch switches.  Output compared with the exact
direct-convolution oracle on the same inputs / weights / noise: max-abs on the BEV output, beside the same figure with every eligible
layer in F(2x2, 3x3) (the shipped arithmetic).  Gate: <= 1e-4, the loosest bound an existing test holds on a Winograd result; the
single-layer figures (inputs N(0,1), weights by the law of tests/test_gpu_conv_random.py, 48x48 outputs, against the fp32 direct form)
must stay inside 5e-5, the bound of test_winograd_conv.
Usage: python3 tools/winograd42_study.py [quick]"""
import json
import os
import sys
import time

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools", "r04"))
from oracle import cases, ref_torch as R  # noqa: E402
from workloads import hashfill  # noqa: E402
from util import build_pair  # noqa: E402
import winograd_study as W22  # noqa: E402  (F(2x2, 3x3) restatement; importing it installs ITS shim, replaced below)

MODE = {"plain": None, "n42": 0, "n22": 0, "direct": 0}
_conv2d, _convT = W22._conv2d, W22._convT

BT4 = torch.tensor([[4., 0., -5., 0., 1., 0.], [0., -4., -4., 1., 1., 0.], [0., 4., -4., -1., 1., 0.],
                    [0., -2., -1., 2., 1., 0.], [0., 2., -1., -2., 1., 0.], [0., 4., 0., -5., 0., 1.]])
G4 = torch.tensor([[1 / 4., 0., 0.], [-1 / 6., -1 / 6., -1 / 6.], [-1 / 6., 1 / 6., -1 / 6.],
                   [1 / 24., 1 / 12., 1 / 6.], [1 / 24., -1 / 12., 1 / 6.], [0., 0., 1.]])
AT4 = torch.tensor([[1., 1., 1., 1., 1., 0.], [0., 1., -1., 2., -2., 0.], [0., 1., 1., 4., 4., 0.], [0., 1., -1., 8., -8., 1.]])
BT2, G2, AT2 = W22.BT, W22.G, W22.AT


def winograd42_3x3(x, w):
    """conv2d(x, w, padding=1) for 3x3 w, stride 1, via F(4,3) along y and F(2,3) along x in fp32.  x [N, C, H, W], w [O, C, 3, 3]."""
    N, C, H, Wd = x.shape
    He, We = (H + 3) // 4 * 4, Wd + (Wd & 1)
    xp = F.pad(x, (1, 1 + We - Wd, 1, 1 + He - H))
    d = xp.unfold(2, 6, 4).unfold(3, 4, 2)                       # [N, C, Th, Tw, 6, 4]
    V = torch.einsum("ai,nctuij,bj->nctuab", BT4, d, BT2)
    U = torch.einsum("ai,ocij,bj->ocab", G4, w, G2)              # computed once per layer (pack time)
    Th, Tw = V.shape[2], V.shape[3]
    Vm = V.permute(4, 5, 1, 0, 2, 3).reshape(24, C, N * Th * Tw)
    Um = U.permute(2, 3, 0, 1).reshape(24, w.shape[0], C)
    M = torch.bmm(Um, Vm).reshape(6, 4, w.shape[0], N, Th, Tw)
    Y = torch.einsum("ai,ijontu,bj->notuab", AT4, M, AT2)        # [N, O, Th, Tw, 4, 2]
    Y = Y.permute(0, 1, 2, 4, 3, 5).reshape(N, w.shape[0], 4 * Th, 2 * Tw)
    return Y[:, :, :H, :Wd].contiguous()


def pick(x, w, stride, padding, dilation, groups):
    s = stride if isinstance(stride, int) else stride[0]
    p = padding if isinstance(padding, int) else padding[0]
    d = dilation if isinstance(dilation, int) else dilation[0]
    if groups != 1 or tuple(w.shape[2:]) != (3, 3) or s != 1 or p != d or MODE["plain"] == "direct":
        return None, 0
    return (MODE["plain"] if d == 1 else "f22"), d


class Shim:
    def __getattr__(self, k):
        return getattr(F, k)

    def _run(self, x, w, b, form, d):
        MODE["n42" if form == "f42" else "n22"] += 1
        y = winograd42_3x3(x, w) if form == "f42" else W22.conv3x3_any_dilation(x, w, d)
        return y if b is None else y + b.view(1, -1, 1, 1)

    def conv2d(self, x, w, b=None, stride=1, padding=0, dilation=1, groups=1):
        form, d = pick(x, w, stride, padding, dilation, groups)
        if form is None:
            MODE["direct"] += 1
            return _conv2d(x, w, b, stride, padding, dilation, groups)
        return self._run(x, w, b, form, d)

    def conv_transpose2d(self, x, w, b=None, stride=1, padding=0, *a, **k):
        ok = tuple(w.shape[2:]) == (3, 3) and stride == 1 and padding == 1 and not a and not k and MODE["plain"] != "direct"
        if not ok:
            MODE["direct"] += 1
            return _convT(x, w, b, stride, padding, *a, **k)
        return self._run(x, w.flip(2, 3).transpose(0, 1).contiguous(), b, MODE["plain"], 1)


R.F = Shim()


def forward(C, H, W, ts, solver):
    cts, lts, tts, dt = cases.timeset(ts)
    _, sd = build_pair(C, solver, True, True, dt, device="cpu")
    cam, lid = cases.bev_inputs(C, H, W, cts.shape[1], lts.shape[1])
    with torch.no_grad():
        y, _ = R.future_prediction_ode_forward(sd, cases.present_input(cam, lid), cam, lid, cts, lts, tts, dt, 2, solver, True, True,
                                                hashfill.HashedNoise(cases.EPS_SEED))
    return y


def single_layers():
    """one layer, the data law of tests/test_gpu_conv_random.py: max-abs against the fp32 direct form (and against fp64)"""
    rows = []
    for cin in (64, 128, 256):
        x = hashfill.normal(f"w42_x_{cin}", (2, cin, 48, 48), 1)
        w = hashfill.uniform(f"w42_w_{cin}", (64, cin, 3, 3), -1, 1, 3) * (3.0 / (cin * 9)) ** 0.5
        direct = _conv2d(x, w, None, 1, 1)
        exact = _conv2d(x.double(), w.double(), None, 1, 1)
        row = {"cin": cin, "absmax_of_output": float(direct.abs().max()), "direct_vs_fp64": float((direct - exact).abs().max())}
        for tag, fn in (("f22", W22.winograd_3x3), ("f42", winograd42_3x3)):
            y = fn(x, w)
            row[tag + "_vs_direct"] = float((y - direct).abs().max())
            row[tag + "_vs_fp64"] = float((y - exact).abs().max())
        rows.append(row)
    return rows


def selfcheck():
    g = torch.Generator().manual_seed(0)
    for shape in ((2, 5, 11, 14), (1, 3, 13, 9), (1, 4, 8, 16)):
        x = torch.randn(*shape, generator=g)
        w = torch.randn(7, shape[1], 3, 3, generator=g)
        e = (winograd42_3x3(x, w) - _conv2d(x, w, None, 1, 1)).abs().max()
        assert e < 1e-4, (shape, float(e))


def main():
    quick = len(sys.argv) > 1 and sys.argv[1] == "quick"
    torch.set_num_threads(8)
    selfcheck()
    singles = single_layers()
    print(json.dumps(singles), flush=True)
    runs = [("C=64 BEV 200x200 config 2 shipped euler", 64, 200, 200, "shipped", "euler"),
            ("C=32 BEV 200x200 config 1 euler", 32, 200, 200, "config1", "euler")]
    if not quick:
        runs += [("C=64 BEV 200x200 config 4 future16 euler", 64, 200, 200, "future16", "euler"),
                 ("C=64 BEV 200x200 config 5 stream40 (46 steps) euler", 64, 200, 200, "stream40", "euler")]
    rows = []
    out_path = os.path.join(ROOT, "profiles", "winograd42_accuracy_study.json")
    for name, C, H, W, ts, solver in runs:
        t0 = time.time()
        MODE.update(plain="direct")
        ref = forward(C, H, W, ts, solver)
        row = {"case": name, "absmax_of_output": float(ref.abs().max())}
        for tag, plain in (("plain_f42_dilated_f22", "f42"), ("all_f22_as_shipped", "f22")):
            MODE.update(plain=plain, n42=0, n22=0, direct=0)
            y = forward(C, H, W, ts, solver)
            row[tag] = {"maxabs": float((y - ref).abs().max()), "layers_f42": MODE["n42"], "layers_f22": MODE["n22"], "layers_direct": MODE["direct"]}
        row["seconds"] = time.time() - t0
        rows.append(row)
        print(json.dumps(row), flush=True)
        worst = max(r["plain_f42_dilated_f22"]["maxabs"] for r in rows)
        json.dump({"what": __doc__.split("Usage")[0], "gate": "<= 1e-4 max-abs on the BEV output; single layers <= 5e-5 against the direct form",
                   "single_layers": singles, "worst_single_layer_vs_direct": max(r["f42_vs_direct"] for r in singles),
                   "worst_bev_maxabs": worst, "inside_the_gate": bool(worst <= 1e-4 and max(r["f42_vs_direct"] for r in singles) <= 5e-5),
                   "rows": rows}, open(out_path, "w"), indent=1)


if __name__ == "__main__":
    main()
