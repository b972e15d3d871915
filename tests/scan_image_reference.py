"""Plain numpy statement of the scan images (fpe_scan_*_image*; include/fpe.h, point 6 of the scan block): which pixels of a depth or
range image are points, and the three floats of each by the contract's f32 rule — every operation one np.float32 operation, rounded
on its own, the divisions true divisions.  Everything downstream of the points is the existing contract: fuse, clear and close here are
calls of tests/scan_reference.py, tests/scan_clear_reference.py and tests/scan_close_reference.py on points(im, image).  A descriptor is
a dict with the fields of fpe_scan_image (planner.make_scan_image takes it as keywords); an image is a (height, row_pitch) array of
uint16 or float32.  The cases the CPU and the GPU tests share are built here: each is a dict with sr.main_case's keys, `points` being
points(im, image), plus `image` and `im`.  numpy only; no engine code."""
import numpy as np

from tests import scan_clear_reference as cr
from tests import scan_close_reference as kr
from tests import scan_reference as sr

F32, F64 = np.float32, np.float64
NAN = np.array([0x7FC00000], np.uint32).view(F32)[0]  # the point of an invalid pixel, three times
MAX_POINTS = 1 << 22


def descriptor(model, format, width, height, row_pitch=None, row_step=1, col_step=1, depth_scale=1.0, fx=1.0, fy=1.0, cx=0.0, cy=0.0,
               row_dir=None, col_dir=None):
    return dict(model=model, format=format, width=int(width), height=int(height), row_pitch=int(width if row_pitch is None else row_pitch),
                row_step=int(row_step), col_step=int(col_step), depth_scale=F32(depth_scale), fx=F32(fx), fy=F32(fy), cx=F32(cx), cy=F32(cy),
                row_dir=None if row_dir is None else np.ascontiguousarray(row_dir, F32), col_dir=None if col_dir is None else np.ascontiguousarray(col_dir, F32))


def selected(im):
    """(rows v, columns u) of the selected pixels; the point ordinal of (v[ri], u[ci]) is ri * len(u) + ci."""
    return np.arange(0, im["height"], im["row_step"]), np.arange(0, im["width"], im["col_step"])


def points(im, image, reciprocal=False):
    """The (n_sel, 3) float32 points of the image.  reciprocal: the WRONG pinhole rule that multiplies by a rounded 1 / fx and 1 / fy
    (for the CPU test's claim that it can tell the two apart)."""
    v, u = selected(im)
    flat = np.ascontiguousarray(image).reshape(-1)
    raw = flat[v[:, None] * im["row_pitch"] + u[None, :]]
    scale = F32(im["depth_scale"])
    with np.errstate(all="ignore"):
        if im["format"] == "u16":
            assert raw.dtype == np.uint16
            valid = raw != 0
            d = raw.astype(F32) * scale
        else:
            assert raw.dtype == F32
            valid = np.isfinite(raw) & (raw > 0)
            d = raw * scale
        if im["model"] == "pinhole":
            xn = (u.astype(F32)[None, :] - F32(im["cx"])) * d
            yn = (v.astype(F32)[:, None] - F32(im["cy"])) * d
            if reciprocal:
                x, y = xn * (F32(1) / F32(im["fx"])), yn * (F32(1) / F32(im["fy"]))
            else:
                x, y = xn / F32(im["fx"]), yn / F32(im["fy"])
            z = d
        else:
            rd, cd = np.asarray(im["row_dir"], F32).reshape(-1, 2), np.asarray(im["col_dir"], F32).reshape(-1, 2)
            ce, se = rd[v, 0][:, None], rd[v, 1][:, None]
            ca, sa = cd[u, 0][None, :], cd[u, 1][None, :]
            w = d * ce
            x, y, z = w * ca, w * sa, d * se
    assert all(a.dtype == F32 for a in (d, x, y, z))
    out = np.stack([np.broadcast_to(a, valid.shape) for a in (x, y, z)], axis=-1).reshape(-1, 3).copy()
    out[~valid.reshape(-1)] = NAN
    return out


# Everything downstream is the existing contract on points(im, image): nothing is restated.
def fuse(case, **kw):
    return sr.run(case, **kw)


def clear(case, **kw):
    return cr.run(case, **kw)


def close(elev, kp=None, rect=None):
    return kr.close(elev, kp, rect)


# Descriptor fields that are refused whatever the rest of a valid pinhole descriptor of at least 8 x 6 pixels says (a null table of
# the spherical model and a non-zero reserved word are refused too: the tests make those by hand).
REFUSED = {
    "model 2": dict(model=2), "model -1": dict(model=-1), "format 2": dict(format=2), "format -1": dict(format=-1),
    "width 0": dict(width=0), "width 4097": dict(width=4097, row_pitch=4097), "height 0": dict(height=0), "height 4097": dict(height=4097),
    "pitch below width": dict(row_pitch=7), "row_step 0": dict(row_step=0), "col_step 0": dict(col_step=0), "row_step -1": dict(row_step=-1),
    "scale 0": dict(depth_scale=0.0), "scale negative": dict(depth_scale=-0.001), "scale NaN": dict(depth_scale=np.nan), "scale inf": dict(depth_scale=np.inf),
    "fx 0": dict(fx=0.0), "fx -0": dict(fx=-0.0), "fy 0": dict(fy=0.0), "fx NaN": dict(fx=np.nan), "fy inf": dict(fy=np.inf),
    "cx NaN": dict(cx=np.nan), "cy inf": dict(cy=-np.inf),
    "more than FPE_SCAN_MAX_POINTS": dict(width=4096, height=1025, row_pitch=4096),
}

# ---- the cases -------------------------------------------------------------------------------------------------------------------
WIDTH, HEIGHT = 160, 120
SENTINEL_U16, SENTINEL_F32 = np.uint16(1234), F32(1.234)  # the padding of a pitched image: it would be a valid depth


def _case(name, pos, T, im, image, replace_count=7, seed=1):
    rows, cols = sr.MAPS[name]
    e0, v0 = sr.prior_layers(rows, cols, pos, pos, seed + 4)
    return dict(rows=rows, cols=cols, res=sr.RES, pos=tuple(pos), T=np.asarray(T, F64).reshape(12), points=points(im, image), roi=(0, 0, rows, cols),
                params=sr.params(replace_count=replace_count, min_z=-1.0, max_z=2.0), elev=e0, var=v0, stride=3, image=image, im=im)


def _padded(img, pad, sentinel):
    if not pad:
        return np.ascontiguousarray(img)
    out = np.full((img.shape[0], img.shape[1] + pad), sentinel, img.dtype)
    out[:, :img.shape[1]] = img
    return out


def _depth_scene(name, pos, yaw, pitch, seed):
    """The transform, the focal length (as main_case derives it) and the z of sr.pinhole_scan's points as a (HEIGHT, WIDTH) f64 image."""
    rows, cols = sr.MAPS[name]
    g = sr.geometry(rows, cols, sr.RES, pos)
    T = sr.look_down((pos[0] + 0.05, pos[1] - 0.03, 1.2), yaw, pitch)
    focal = WIDTH * 1.2 / (0.9 * min(g["lenX"], g["lenY"]))
    z = sr.pinhole_scan(T, WIDTH, HEIGHT, focal, pos, seed)[:, 2].astype(F64).reshape(HEIGHT, WIDTH)
    return T, focal, z


def depth_u16(name="100x72", pos=(0.0, 0.0), yaw=0.3, pitch=0.0, steps=(1, 1), pad=0, seed=1):
    """A depth camera looking down from 1.2 m: millimetres as uint16, pixels of every drop class planted."""
    T, focal, z = _depth_scene(name, pos, yaw, pitch, seed)
    img = np.rint(z * 1000.0).astype(np.uint16)
    img[0, 0] = img[5, 7] = 0       # invalid
    img[0, 1], img[0, 2] = 65535, 50  # range: too far, too near
    img[0, 3] = 3000                # height: below min_z
    img[119, 159] = 2100            # off the map
    im = descriptor("pinhole", "u16", WIDTH, HEIGHT, WIDTH + pad, steps[0], steps[1], 0.001, focal, focal, 0.5 * (WIDTH - 1), 0.5 * (HEIGHT - 1))
    return _case(name, pos, T, im, _padded(img, pad, SENTINEL_U16), seed=seed)


def depth_f32(name="100x72", pos=(0.0, 0.0), yaw=0.3, pitch=0.0, steps=(1, 1), pad=0, seed=1):
    """The same scene as floats in metres (scale 1), with NaN, +infinity, 0, -0 and a negative pixel planted."""
    T, focal, z = _depth_scene(name, pos, yaw, pitch, seed)
    img = z.astype(F32)
    img[0, 0], img[5, 7], img[9, 9], img[9, 10], img[9, 11] = np.nan, np.inf, 0.0, -0.0, -1.25
    img[0, 1], img[0, 2], img[0, 3], img[119, 159] = 65.535, 0.05, 3.0, 2.1
    im = descriptor("pinhole", "f32", WIDTH, HEIGHT, WIDTH + pad, steps[0], steps[1], 1.0, focal, focal, 0.5 * (WIDTH - 1), 0.5 * (HEIGHT - 1))
    return _case(name, pos, T, im, _padded(img, pad, SENTINEL_F32), seed=seed)


RINGS, AZIMUTHS = 16, 256


def lidar_f32(name="100x72", pos=(0.0, 0.0), seed=1):
    """A spinning lidar 0.6 m up (sensor frame = map axes): 16 rings from -40 to -5 degrees, 256 azimuths, ranges in metres as floats.
    The far rings leave the map.  The tables are numpy's cosines and sines cast to f32; one entry is NaN."""
    rng = np.random.default_rng(seed)
    cam = np.array([pos[0] + 0.05, pos[1] - 0.03, 0.6])
    T = np.hstack([np.eye(3), cam.reshape(3, 1)])
    el = np.deg2rad(np.linspace(-40.0, -5.0, RINGS))
    az = 2.0 * np.pi * np.arange(AZIMUTHS) / AZIMUTHS
    d = np.stack([np.cos(el)[:, None] * np.cos(az)[None, :], np.cos(el)[:, None] * np.sin(az)[None, :], np.sin(el)[:, None] * np.ones(AZIMUTHS)[None, :]], -1)
    r = -cam[2] / d[..., 2]
    for _ in range(2):  # the plane z = 0 first, then the terrain's height there
        hit = cam + r[..., None] * d
        r = (sr.terrain_height(hit[..., 0], hit[..., 1], pos) - cam[2]) / d[..., 2]
    img = (r + 0.001 * rng.standard_normal(r.shape)).astype(F32)
    row_dir = np.stack([np.cos(el), np.sin(el)], 1).astype(F32)
    col_dir = np.stack([np.cos(az), np.sin(az)], 1).astype(F32)
    col_dir[5, 0] = np.nan
    im = descriptor("spherical", "f32", AZIMUTHS, RINGS, row_dir=row_dir, col_dir=col_dir)
    return _case(name, pos, T, im, img, seed=seed)


def far_pitched():
    """depth_u16 far from the origin, yawed and pitched: a contracted multiply-add in the transform would change bits here."""
    return depth_u16("100x72", pos=sr.FAR_POS, yaw=0.3, pitch=0.2, seed=31)


def one_cell():
    """64 x 64 spherical pixels that all look straight down: 4 096 points in ONE cell, ranges one raw unit (20 micrometres) apart — runs
    of equal cells cross every wavefront and every row end, and the top 5 cm of the 8 cm are kept."""
    pos = (0.0, 0.0)
    T = np.hstack([np.eye(3), np.array([[pos[0] + 0.05], [pos[1] - 0.03], [1.2]])])
    img = (57000 + np.random.default_rng(5).permutation(4096)).astype(np.uint16).reshape(64, 64)
    down = np.array([np.cos(-0.5 * np.pi), np.sin(-0.5 * np.pi)])
    im = descriptor("spherical", "u16", 64, 64, depth_scale=2e-5, row_dir=np.tile(down, (64, 1)), col_dir=np.tile([1.0, 0.0], (64, 1)))
    return _case("100x72", pos, T, im, img)


def one_row(width=64):
    """A 1 x width pinhole image whose pixels are one cell apart on the ground: one point per cell along a line of cells."""
    pos = (0.0, 0.0)
    T = sr.look_down((pos[0] + 0.05, pos[1] - 0.03, 1.2), 0.0, 0.0)
    img = np.full((1, width), 1200, np.uint16)
    im = descriptor("pinhole", "u16", width, 1, depth_scale=0.001, fx=60.0, fy=60.0, cx=0.5 * width, cy=0.0)
    return _case("100x72", pos, T, im, img)


EDGE_WIDTHS = (1, 63, 64, 65, 255, 256, 257)


def launch_edge(width, height=1, pitch=None):
    """Small images around a wavefront and a workgroup.  One row: pixels 5 mm apart on the ground, so neighbouring lanes share cells.
    Two rows (row_pitch 70): every pixel in one cell, depths a millimetre apart — the run of equal cells spans the row end."""
    pos = (0.0, 0.0)
    T = sr.look_down((pos[0] + 0.05, pos[1] - 0.03, 1.2), 0.3, 0.0)
    f = 240.0 if height == 1 else 1.0e6
    img = (1100 + (np.arange(width * height) * 7) % 97).astype(np.uint16).reshape(height, width)
    pad = 0 if pitch is None else pitch - width
    im = descriptor("pinhole", "u16", width, height, width + pad, depth_scale=0.001, fx=f, fy=f, cx=0.5 * (width - 1), cy=0.5 * (height - 1))
    return _case("100x72", pos, T, im, _padded(img, pad, SENTINEL_U16))


def edge_cases():
    cases = {f"1x{w}": launch_edge(w) for w in EDGE_WIDTHS}
    cases["2x64,pitch70"] = launch_edge(64, 2, 70)
    cases["2x65,pitch70"] = launch_edge(65, 2, 70)
    return cases


def main_cases():
    """Cases 1 - 5 of the GPU tests, on both maps where the case is about the map."""
    return {
        "depth_u16,100x72": depth_u16("100x72"),
        "depth_u16,48x40": depth_u16("48x40"),
        "depth_u16,steps(2,3)": depth_u16("100x72", steps=(2, 3)),
        "depth_u16,pitch+7": depth_u16("48x40", pad=7),
        "depth_f32": depth_f32("100x72"),
        "depth_f32,steps(2,3),pitch+7": depth_f32("48x40", steps=(2, 3), pad=7),
        "lidar_f32,100x72": lidar_f32("100x72"),
        "lidar_f32,48x40": lidar_f32("48x40"),
        "far,pitched": far_pitched(),
    }


def contention_cases():
    return {"one cell": one_cell(), "one row": one_row()}


def all_cases():
    return {**main_cases(), **contention_cases(), **edge_cases()}
