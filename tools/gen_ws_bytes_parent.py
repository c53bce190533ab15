"""Record what the workspace size queries of the model entry points return: tests/golden/ws_bytes_parent.json.

Run against the PARENT commit's library (SF_LIB_PATH=/path/to/parent/libsfnative.so python tools/gen_ws_bytes_parent.py COMMIT): the
fixture pins that no query of the branch returns more than the parent's did (tests/test_workspace_layout.py).  The size functions are
host arithmetic: no GPU is needed.  Every record is {fn, args, flow, bytes}; `flow` is the persistent-flow mode (sf_set_flow_mode) in
force at the query, recorded off and on for the queries that see it."""
import json
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))

SHAPES = [(64, 1, 8, 16), (64, 3, 20, 36), (64, 1, 50, 50), (64, 1, 96, 96), (64, 4, 60, 60), (128, 1, 50, 50), (64, 32, 50, 50)]
HID = 128      # DeepLab head; the camera neck's twin head is 2 x 64
FLOW_QUERIES = ("sf_ode_step_ws_bytes", "sf_nnfo_rollout_ws_bytes")


def queries(C, n, H, W):
    """(function, arguments) of every covered size query at one (C, n, H, W)."""
    q = [(f, (C, n, H, W)) for f in ("sf_gru_cell_ws_bytes", "sf_spatial_gru_ws_bytes", "sf_dual_cell_ws_bytes", "sf_infer_state_ws_bytes",
                                    "sf_ode_step_ws_bytes", "sf_nnfo_rollout_ws_bytes", "sf_nnfo_rollout_carry_bytes",
                                    "sf_convnext_block_ws_bytes")]
    q += [("sf_channel_mean_ws_bytes", (C, n)), ("sf_dist_head_ws_bytes", (C, n)),
          ("sf_bottleblock_ws_bytes", (C, C, n, H, W)), ("sf_bottleblock_ws_bytes", (2 * C, C, n, H, W)),
          ("sf_bottleneck_ws_bytes", (C, C, n, H, W)), ("sf_bottleneck_ws_bytes", (C, 2 * C, n, H, W)),
          ("sf_small_encoder_ws_bytes", (C, C, n, H, W)), ("sf_small_decoder_ws_bytes", (C, C, n, H, W)),
          ("sf_deeplab_head_ws_bytes", (C, HID, n, H, W)), ("sf_camera_neck_ws_bytes", (C, C // 2, 64, 48, HID, n, H, W))]
    return q


def main():
    from streamingflow_amd import _lib
    L = _lib.lib()
    records = [{"fn": "sf_conv2d_ex_ws_bytes", "args": [], "flow": 0, "bytes": int(L.sf_conv2d_ex_ws_bytes())}]
    was = L.sf_set_flow_mode(0)
    for shape in SHAPES:
        for fn, args in queries(*shape):
            for flow in (0, 1) if fn in FLOW_QUERIES else (0,):
                L.sf_set_flow_mode(flow)
                records.append({"fn": fn, "args": list(args), "flow": flow, "bytes": int(getattr(L, fn)(*args))})
                L.sf_set_flow_mode(0)
    L.sf_set_flow_mode(was)
    commit = sys.argv[1] if len(sys.argv) > 1 else "unknown"
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tests", "golden", "ws_bytes_parent.json")
    with open(path, "w") as f:      # one record per line
        f.write('{"commit": %s, "shapes": %s, "records": [\n' % (json.dumps(commit), json.dumps([list(s) for s in SHAPES])))
        f.write(",\n".join(json.dumps(r) for r in records))
        f.write("\n]}\n")
    print("%d records -> %s" % (len(records), os.path.normpath(path)))


if __name__ == "__main__":
    main()
