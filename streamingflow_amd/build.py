"""Build libsfnative.so (HIP, gfx950) in-tree with hipcc.  `python -m streamingflow_amd.build`."""
import os
import subprocess
import sys
from concurrent.futures import ThreadPoolExecutor

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "csrc")
LIB = os.path.join(HERE, "libsfnative.so")
SOURCES = ["conv_igemm.hip", "conv_sp.hip", "conv_wino.hip", "convnext_mlp.hip", "aux_kernels.hip", "dispatch.hip", "api.hip", "lift_splat.hip", "rig_affines.hip", "camera_neck.hip", "effnet.hip", "image_frontend.hip", "voxelize.hip", "sparse_index.hip", "eval_kernels.hip", "instance_track.hip", "panoptic_score.hip", "plan_kernels.hip", "plan_sampler.hip", "flow_warp.hip", "pack.hip"]
FLAGS = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-fno-gpu-rdc", "-Wall", "-Wno-unused-function"]


def _stale(out, deps):
    if not os.path.exists(out):
        return True
    t = os.path.getmtime(out)
    return any(os.path.getmtime(d) > t for d in deps)


def build(force=False, verbose=False):
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    if not os.path.exists(hipcc):
        hipcc = "hipcc"
    headers = [os.path.join(CSRC, h) for h in ("sf_device.h", "sf_math.h", "sf_launch.h", "dispatch.h", "fresnel_tables.h")] + [os.path.join(HERE, "..", "include", h) for h in ("sfnative.h", "sfnative_effnet.h")]
    objs, jobs = [], []
    for src in SOURCES:
        s = os.path.join(CSRC, src)
        o = os.path.join(CSRC, src.replace(".hip", ".o"))
        objs.append(o)
        if force or _stale(o, [s] + headers):
            jobs.append([hipcc] + FLAGS + ["-c", s, "-o", o])

    def run(cmd):
        if verbose:
            print(" ".join(cmd), flush=True)
        r = subprocess.run(cmd, capture_output=True, text=True)
        if r.returncode != 0:
            raise RuntimeError("hipcc failed:\n%s\n%s" % (" ".join(cmd), r.stderr))
        if verbose and r.stderr.strip():
            print(r.stderr)
        return r.stderr

    if jobs:
        with ThreadPoolExecutor(max_workers=7) as ex:
            list(ex.map(run, jobs))
    if jobs or force or _stale(LIB, objs):
        run([hipcc, "--offload-arch=gfx950", "-shared", "-fPIC", "-o", LIB] + objs)
    return LIB


if __name__ == "__main__":
    print(build(force="--force" in sys.argv, verbose=True))
