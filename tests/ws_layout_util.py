"""Shared by test_workspace_layout.py (CPU) and test_gpu_workspace_exact.py: every model entry point that carves a workspace, as
(size query, call) pairs on given weight structs and tensor pointers.  The CPU test hands over placeholder descriptors and pointers
(a refused call never reads them), the GPU test the packed weights of real modules and real tensors."""
import ctypes
import types

from streamingflow_amd import _lib

HOLE = ctypes.c_void_p(4096)      # placeholder pointer: never dereferenced
HID = 128
NAMES = ("bottleblock", "bottleblock_proj", "bottleneck_down0", "bottleneck_down1", "camera_neck", "channel_mean", "convnext_block",
         "deeplab_head", "deeplab_head_planar", "dist_head_pool0", "dist_head_pool1", "dual_cell", "gru_cell", "gru_ode_cell", "infer_state",
         "infer_state_philox", "ode_step_euler", "ode_step_rk4", "rollout", "rollout_philox", "rollout_resume", "rollout_resume_philox",
         "small_decoder", "small_encoder", "spatial_gru", "trust_mix")


def conv(cout, c0, c1=0, k=1):
    """A valid descriptor (csrc/api.hip: valid_w) with placeholder weights: a refusal that was missed must end as a failed launch,
    not as a division by a zero stride."""
    w = _lib.ConvW()
    w.w = w.scale = w.bias = HOLE.value
    w.cout, w.cout_pad, w.c0, w.c1, w.cin_pad = cout, (cout + 15) // 16 * 16, c0, c1, (c0 + c1 + 31) // 32 * 32
    w.kh = w.kw = k
    w.dil = w.stride = 1
    w.pad = (k - 1) // 2
    return w


def _res(cin, cout):
    w = _lib.ResW()
    w.conv1, w.conv2 = conv(cin, cin, 0, 3), conv(cout, cin, 0, 3)
    if cin != cout:
        w.proj = conv(cout, cin)
    return w


def _deeplab(C, hid, cls):
    w = _lib.DeepLabW()
    w.branch[0] = conv(hid, C)
    for i in (1, 2, 3):
        w.branch[i] = conv(hid, C, 0, 3)
    w.pool_w = w.pool_scale = w.pool_bias = w.proj_pool_w = HOLE.value
    w.project, w.conv3, w.cls, w.C, w.hid = conv(hid, 4 * hid), conv(hid, hid, 0, 3), conv(cls, hid), C, hid
    return w


def placeholder_weights(C):
    """The weight structs of every module at C channels, valid descriptors around placeholder pointers."""
    W = types.SimpleNamespace()
    W.gru = _lib.GruW()
    W.gru.gates, W.gru.cand = conv(2 * C, C, C, 3), conv(C, C, C, 3)
    d = W.dual = _lib.DualW()
    d.gates1, d.cand1, d.gates2, d.cand2, d.dec2 = conv(2 * C, C, C, 3), conv(C, C, C, 3), conv(2 * C, C, 0, 3), conv(C, C, C, 3), conv(C, C)
    d.tg7, d.tgproj, d.tg1, d.tg3 = conv(C, C, C, 7), conv(C, C, C), conv(C, C), conv(2 * C, C, 0, 3)
    d.w_logit, d.C = HOLE.value, C
    p = W.pm = _lib.PModelW()
    p.rb0, p.rb1, p.last, p.C = _res(C, 2 * C), _res(2 * C, 2 * C), conv(2 * C, 2 * C, 0, 3), C
    p.se0_fc0 = p.se0_fc2 = p.se1_fc0 = p.se1_fc2 = HOLE.value
    W.bottle, W.bottle_proj = _lib.BottleW(), _lib.BottleW()
    W.bottle.c7, W.bottle.c1, W.bottle.c3 = conv(C // 2, C, 0, 7), conv(C // 2, C // 2), conv(C, C // 2, 0, 3)
    W.bottle_proj.c7, W.bottle_proj.c1, W.bottle_proj.c3, W.bottle_proj.proj = conv(C, C, C, 7), conv(C, C), conv(C, C, 0, 3), conv(C, C, C)
    W.enc, W.dec = _lib.EncoderW(), _lib.DecoderW()
    for i, (ci, co) in enumerate([(C, C), (C, 2 * C), (2 * C, 2 * C), (2 * C, 2 * C), (2 * C, 4 * C)]):
        W.enc.blocks[i] = _res(ci, co)
    W.enc.last, W.enc.C, W.enc.F = conv(C, 4 * C, 0, 3), C, C
    for i, (ci, co) in enumerate([(4 * C, 2 * C), (2 * C, 2 * C), (2 * C, 2 * C), (2 * C, C), (C, C)]):
        W.dec.blocks[i] = _res(ci, co)
    W.dec.first, W.dec.last0, W.dec.last1, W.dec.C, W.dec.F = conv(4 * C, C, 0, 3), conv(C, C, 0, 3), conv(C, C, 0, 3), C, C
    W.bottlenecks = []
    for down in (0, 1):
        b = _lib.BottleneckW()
        b.down, b.conv, b.up, b.proj, b.downsample = conv(C // 2, C), conv(C // 2, C // 2, 0, 3), conv(2 * C, C // 2), conv(2 * C, C), down
        b.conv.stride = 2 if down else 1
        W.bottlenecks.append(b)
    W.dist = conv(2 * 32, C)
    c = W.convnext = _lib.ConvNextW()
    c.dw_w = c.dw_b = c.ln_w = c.ln_b = HOLE.value
    c.pw1, c.pw2, c.C = conv(4 * C, C), conv(C, 4 * C), C
    W.deeplab = _deeplab(C, HID, 8)
    W.twin = _deeplab(C, HID, 2 * C)
    W.neck_convs = (_lib.ConvW * 4)(conv(64, C // 2, C, 3), conv(64, 64, 0, 3), conv(48, C // 2, C, 3), conv(48, 48, 0, 3))
    return W


def entry_points(W, X, Y, n, H, Wd):
    """name -> (queried bytes, call(ws, ws_bytes) -> status) of every covered entry point on the weight structs `W`; X / Y: the pointer
    handed over for every input / output tensor.  The size queries get what each call derives from its own weights."""
    L = _lib.lib()
    P = ctypes.byref
    C = W.dual.C
    ops = (ctypes.c_int32 * 4)(_lib.OP_JUMP, 0, _lib.OP_STEP, 0)
    sel = (ctypes.c_int32 * 1)(2)
    e = {}
    Cg = W.gru.cand.cout
    e["channel_mean"] = (L.sf_channel_mean_ws_bytes(C, n), lambda ws, b: L.sf_channel_mean_fwd(X, Y, n, H * Wd, C, ws, b, None))
    e["gru_cell"] = (L.sf_gru_cell_ws_bytes(Cg, n, H, Wd), lambda ws, b: L.sf_gru_cell_fwd(P(W.gru), X, X, Y, n, H, Wd, ws, b, None))
    e["gru_ode_cell"] = (L.sf_gru_cell_ws_bytes(Cg, n, H, Wd), lambda ws, b: L.sf_gru_ode_cell_fwd(P(W.gru), X, X, Y, n, H, Wd, ws, b, None))
    e["spatial_gru"] = (L.sf_spatial_gru_ws_bytes(Cg, n, H, Wd), lambda ws, b: L.sf_spatial_gru_fwd(P(W.gru), X, X, Y, 2, n, H, Wd, ws, b, None))
    e["dual_cell"] = (L.sf_dual_cell_ws_bytes(C, n, H, Wd),
                      lambda ws, b: L.sf_dual_cell_fwd(P(W.dual), X, X, Y, 0, None, None, None, 0, n, H, Wd, ws, b, None))
    e["trust_mix"] = (L.sf_dual_cell_ws_bytes(C, n, H, Wd),
                      lambda ws, b: L.sf_trust_mix_fwd(P(W.dual), X, X, X, Y, 0, None, None, n, H, Wd, ws, b, None))
    for name, bw, x1 in (("bottleblock", W.bottle, None), ("bottleblock_proj", W.bottle_proj, X)):
        e[name] = (L.sf_bottleblock_ws_bytes(bw.c7.c0 + bw.c7.c1, bw.c3.cout, n, H, Wd),
                   lambda ws, b, bw=bw, x1=x1: L.sf_bottleblock_fwd(P(bw), X, x1, Y, n, H, Wd, ws, b, None))
    e["infer_state"] = (L.sf_infer_state_ws_bytes(C, n, H, Wd), lambda ws, b: L.sf_infer_state_fwd(P(W.pm), X, X, Y, None, n, H, Wd, ws, b, None))
    e["infer_state_philox"] = (L.sf_infer_state_ws_bytes(C, n, H, Wd),
                               lambda ws, b: L.sf_infer_state_philox_fwd(P(W.pm), X, X, 0, Y, None, n, H, Wd, ws, b, None))
    for solver in ("euler", "rk4"):
        e["ode_step_" + solver] = (L.sf_ode_step_ws_bytes(C, n, H, Wd), lambda ws, b, s=_lib.SOLVER[solver]: L.sf_ode_step_fwd(
            P(W.dual), P(W.pm), s, 1, X, X, X, X, Y, Y, n, H, Wd, ws, b, None))
    roll = (P(W.dual), P(W.dual), P(W.pm), _lib.SOLVER["midpoint"], 1, ops, 2, X, X, X, 0, sel, 1, Y, Y)
    seg = (X, X, None, 0, Y, None)      # state_in, p_in, carry_in, draw_base, p_out, carry_out
    need = L.sf_nnfo_rollout_ws_bytes(C, n, H, Wd)
    e["rollout"] = (need, lambda ws, b: L.sf_nnfo_rollout_fwd(*roll, n, H, Wd, ws, b, None))
    e["rollout_philox"] = (need, lambda ws, b: L.sf_nnfo_rollout_philox_fwd(*roll, n, H, Wd, ws, b, None))
    e["rollout_resume"] = (need, lambda ws, b: L.sf_nnfo_rollout_resume_fwd(*roll, *seg, n, H, Wd, ws, b, None))
    e["rollout_resume_philox"] = (need, lambda ws, b: L.sf_nnfo_rollout_resume_philox_fwd(*roll, *seg, n, H, Wd, ws, b, None))
    e["small_encoder"] = (L.sf_small_encoder_ws_bytes(W.enc.C, W.enc.F, n, H, Wd),
                          lambda ws, b: L.sf_small_encoder_fwd(P(W.enc), X, Y, n, H, Wd, ws, b, None))
    e["small_decoder"] = (L.sf_small_decoder_ws_bytes(W.dec.C, W.dec.F, n, H, Wd),
                          lambda ws, b: L.sf_small_decoder_fwd(P(W.dec), X, Y, n, H, Wd, ws, b, None))
    for bn in W.bottlenecks:
        e["bottleneck_down%d" % bn.downsample] = (L.sf_bottleneck_ws_bytes(bn.down.c0, bn.up.cout, n, H, Wd),
                                                  lambda ws, b, bn=bn: L.sf_bottleneck_fwd(P(bn), X, Y, n, H, Wd, ws, b, None))
    for pool in (0, 1):
        e["dist_head_pool%d" % pool] = (L.sf_dist_head_ws_bytes(W.dist.c0, n), lambda ws, b, pool=pool: L.sf_dist_head_fwd(
            P(W.dist), X, Y, n, H, Wd, pool, 1, -5.0, 5.0, ws, b, None))
    e["convnext_block"] = (L.sf_convnext_block_ws_bytes(W.convnext.C, n, H, Wd),
                           lambda ws, b: L.sf_convnext_block_fwd(P(W.convnext), X, Y, n, H, Wd, ws, b, None))
    dl = W.deeplab
    e["deeplab_head"] = (L.sf_deeplab_head_ws_bytes(dl.C, dl.hid, n, H, Wd), lambda ws, b: L.sf_deeplab_head_fwd(P(dl), X, Y, n, H, Wd, ws, b, None))
    e["deeplab_head_planar"] = (L.sf_deeplab_head_ws_bytes(dl.C, dl.hid, n, H, Wd), lambda ws, b: L.sf_deeplab_head_planar_fwd(
        P(dl), X, Y, n, H, Wd, 1, dl.cls.cout * H * Wd, dl.cls.cout * H * Wd, ws, b, None))
    cv = W.neck_convs
    e["camera_neck"] = (L.sf_camera_neck_ws_bytes(W.twin.C, cv[0].c0, cv[1].cout, cv[3].cout, W.twin.hid, n, H, Wd),
                        lambda ws, b: L.sf_camera_neck_fwd(P(W.twin), cv, X, X, Y, Y, Y, n, H, Wd, ws, b, None))
    assert sorted(e) == sorted(NAMES)
    return e
