"""bench.py --dump-outputs, host side: what dump_outputs writes for a set of products (no GPU involved)."""
import os

import numpy as np

import bench
from quadrupedal_foothold_planner_amd import _capi


def _products(B=40, n_cycles=3, world=2, seed=5):
    rng = np.random.default_rng(seed)
    nom = np.zeros((B, n_cycles, 4), _capi.FOOTHOLD_DTYPE)
    for f in ("row", "col"):
        nom[f] = rng.integers(-300, 5000, nom.shape)
    for f in ("x", "y"):
        nom[f] = rng.standard_normal(nom.shape)
    nom["z"] = rng.standard_normal(nom.shape).astype(np.float32)
    nom["z"][0, 0, 0] = np.nan
    nom["valid"], nom["source"] = rng.integers(0, 2, nom.shape), rng.integers(0, 3, nom.shape)
    gathered = np.zeros((world, B, n_cycles, 4), _capi.SELECTED_DTYPE)
    gathered["row"] = rng.integers(0, 1000, gathered.shape)
    return {"nominal": (nom, 0), "default": (rng.standard_normal((B, n_cycles, 4, 3)), 0),
            "cycle_ok": (rng.integers(0, 2, (B, n_cycles)).astype(np.uint8), 0), "gathered_selected": (gathered, 1)}


def _load(d):
    return {f[:-4]: np.load(os.path.join(d, f)) for f in os.listdir(d) if f.endswith(".npy")}


def test_dump_writes_every_field_exactly_as_float32_or_float64(tmp_path):
    prods = _products()
    written = bench.dump_outputs(str(tmp_path), prods, 40)
    got = _load(tmp_path)
    assert sorted(written) == sorted(k + ".npy" for k in got) and "pose_index" not in got
    nom = prods["nominal"][0]
    for f in nom.dtype.names:
        want = np.float32 if nom.dtype[f] == np.float32 or nom.dtype[f].itemsize == 1 else np.float64
        assert got[f"nominal_{f}"].dtype == want, f
        assert np.array_equal(got[f"nominal_{f}"], nom[f], equal_nan=True), f
    assert got["default"].dtype == np.float64 and np.array_equal(got["default"], prods["default"][0])
    assert got["cycle_ok"].dtype == np.float32 and np.array_equal(got["cycle_ok"], prods["cycle_ok"][0])
    assert got["gathered_selected_row"].shape == (2, 40, 3, 4)


def test_dump_over_the_limit_writes_a_fixed_sample_of_the_poses(tmp_path):
    prods = _products()
    bench.dump_outputs(str(tmp_path / "all"), prods, 40)
    limit = sum(p.stat().st_size for p in (tmp_path / "all").iterdir()) // 3
    a, b = tmp_path / "a", tmp_path / "b"
    bench.dump_outputs(str(a), prods, 40, limit=limit)
    bench.dump_outputs(str(b), prods, 40, limit=limit)
    got, again = _load(a), _load(b)
    assert sum(p.stat().st_size for p in a.iterdir()) <= limit
    idx = got["pose_index"].astype(np.int64)
    assert 0 < idx.size < 40 and np.all(np.diff(idx) > 0)
    for k in got:  # same sample every time
        assert np.array_equal(got[k], again[k], equal_nan=True), k
    nom = prods["nominal"][0]
    assert np.array_equal(got["nominal_x"], nom["x"][idx]) and np.array_equal(got["default"], prods["default"][0][idx])
    assert np.array_equal(got["gathered_selected_row"], prods["gathered_selected"][0]["row"][:, idx])
    # a later dump into the same directory leaves its own set only: no pose_index.npy of the sampled one
    (a / "notes.txt").write_text("kept")
    bench.dump_outputs(str(a), prods, 40)
    assert sorted(_load(a)) == sorted(_load(tmp_path / "all")) and (a / "notes.txt").read_text() == "kept"
