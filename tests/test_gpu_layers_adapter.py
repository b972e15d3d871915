"""Engine::exportLayers of the ROS adapter RUN: tests/probe/layers_run.cpp compiled with g++ against the mock grid_map types of
tests/probe/ros_mock (as test_gpu_ros_adapter.py compiles adapter_run.cpp), linked with the real libfpe.so and run on the GPU for
one column-major map with a nonzero start index.  The checksums it prints of every layer's 32-bit patterns must equal the
checksums of the arrays the Python binding returns for the same call."""
import os
import subprocess

import numpy as np
import pytest

from quadrupedal_foothold_planner_amd import _capi, synth
from quadrupedal_foothold_planner_amd import build as fbuild
from quadrupedal_foothold_planner_amd.planner import FootholdPlanner

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def build_driver():
    lib = fbuild.build_engine()
    out_dir = os.path.join(ROOT, "tests", "probe", "_build")
    os.makedirs(out_dir, exist_ok=True)
    exe = os.path.join(out_dir, "layers_run")
    cmd = ["g++", "-std=c++14", "-O1", "-Wall", "-DFPE_WITH_ROS", "-I" + os.path.join(ROOT, "tests", "probe", "ros_mock"),
           "-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(ROOT, "quadrupedal_foothold_planner_amd", "csrc", "ros_adapter"),
           os.path.join(ROOT, "tests", "probe", "layers_run.cpp"), "-o", exe, "-L" + os.path.dirname(lib), "-l:" + os.path.basename(lib),
           "-Wl,-rpath," + os.path.dirname(lib), "-Wl,--allow-shlib-undefined"]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return exe


def checksums(a):
    u = a.reshape(-1).view(np.uint32).astype(np.uint64)
    with np.errstate(over="ignore"):
        return int(u.sum(dtype=np.uint64)), int((u * np.arange(1, u.size + 1, dtype=np.uint64)).sum(dtype=np.uint64))


def test_export_layers_of_the_adapter_equals_the_binding(tmp_path):
    exe = build_driver()
    rows, cols, res = 131, 67, 0.02
    trav, elev = synth.rough_map(rows, cols, res, seed=91, bad_frac=0.1)
    position, (si, sj), roi = (1.5, -0.7), (37, 66), (2, 5, 120, 60)
    buf = lambda layer: np.ascontiguousarray(np.roll(np.roll(layer, si, axis=0), sj, axis=1).T).astype(np.float32).tobytes()  # column-major + start index
    inp = tmp_path / "in.bin"
    with open(inp, "wb") as f:
        f.write(np.array([rows, cols, si, sj, *roi], dtype=np.int32).tobytes())
        f.write(np.array([res, position[0], position[1]], dtype=np.float64).tobytes())
        f.write(buf(trav))
        f.write(buf(elev))
    outp = tmp_path / "out.txt"
    r = subprocess.run([exe, str(inp), str(outp)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (r.returncode, r.stderr[-2000:], open(outp).read()[-500:] if os.path.exists(outp) else "")
    got, mismatch = {}, None
    for ln in open(outp).read().split("\n"):
        t = ln.split()
        if not t:
            continue
        if t[0] == "layer":
            got[int(t[1])] = (int(t[2]), int(t[3]))
        elif t[0] == "mismatch":
            mismatch = int(t[1])
        else:
            raise AssertionError("layers_run: " + ln)
    assert sorted(got) == list(range(_capi.LAYER_COUNT)) and mismatch == 0

    p = FootholdPlanner(0)
    try:
        p.params = _capi.params_yaml()
        p.gridmapCallback(trav, elev, res, position)
        ref = p.export_layers(roi=roi, start_index=(si, sj), storage_order="col")
        for k, name in enumerate(_capi.LAYER_NAMES):
            assert ref[name].shape == (cols, rows)
            assert got[k] == checksums(ref[name]), name
        assert len({got[k] for k in got}) > 5  # (the layers are not all alike: the checksums tell them apart)
    finally:
        p.close()
