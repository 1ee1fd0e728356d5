"""The separable covariance walk (slam_toolbox_amd/csrc/covariance_walk.hpp) against the walk as the reference writes it, bit for
bit and error code for error code, through the stand-alone program tests/covariance_walk_check.cpp (which keeps the as-written double
loop).  No GPU."""
import itertools
import os
import struct
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
KH_OK, KH_ERR_SEARCH = 0, 4
MAX_VARIANCE = 500.0


def hx(v):
    return float(v).hex()


def walk_line(side, resolution, centre, offset, res, w_centre=None, w_offset=None, w_res=None, ang_res=0.01, best_pose=None,
              best_response=0.85, seed=1):
    """one case; the caller's geometry defaults to the search's, the best pose to a point a little off the centre"""
    w_centre = centre if w_centre is None else w_centre
    w_offset = offset if w_offset is None else w_offset
    w_res = res if w_res is None else w_res
    best_pose = (centre[0] + 0.3 * resolution, centre[1] - 0.2 * resolution, 0.1) if best_pose is None else best_pose
    vals = [resolution, centre[0], centre[1], offset[0], offset[1], res[0], res[1], w_centre[0], w_centre[1], w_offset[0], w_offset[1],
            w_res[0], w_res[1], ang_res, best_pose[0], best_pose[1], best_pose[2], best_response, seed]
    return f"walk {side} " + " ".join(hx(v) for v in vals)


# the search lattices: (side, resolution, offsets, resolutions) -> nx x ny
R = 0.005
LATTICES = {
    "1x1": (1, R, (0.0, 0.0), (R, R)),
    "3x3": (3, R, (R, R), (R, R)),
    "5x7": (9, R, (2 * R, 1.5 * R), (R, 0.5 * R)),            # nx != ny, res_x != res_y, the rows on half cells of the grid
    "61x61": (61, R, (0.15, 0.15), (R, R)),                   # the config-2 search
}
SHAPES = {"1x1": (1, 1), "3x3": (3, 3), "5x7": (5, 7), "61x61": (61, 61)}
# centres: the origin, large magnitude either sign, negative, and values whose sums with the pose offsets round
CENTRES = [(0.0, 0.0), (1e3, -1e3), (-1e3 + 0.0025, 1e3 - 0.00125), (-3.7, -12.345678), (0.1 + 0.2, 1.0 / 3.0), (2.5 * R, -0.5 * R)]


@pytest.fixture(scope="module")
def check(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("walk") / "covariance_walk_check")
    subprocess.run(["g++", "-O2", "-std=c++17", "-ffp-contract=off", os.path.join(HERE, "covariance_walk_check.cpp"), "-o", exe], check=True)

    def run(lines):
        r = subprocess.run([exe], input="\n".join(lines) + "\n", capture_output=True, text=True, timeout=60)
        assert r.returncode == 0, r.stdout + r.stderr
        out = [ln.split() for ln in r.stdout.splitlines()]
        assert len(out) == len(lines), r.stdout
        rows = []
        for line, f in zip(lines, out):
            assert len(f) == 22, f
            rc_written, rc_separable, nx, ny = (int(v) for v in f[:4])
            assert rc_written == rc_separable, (line, f)
            assert f[4:13] == f[13:22], (line, f)                # the nine covariance words, bit for bit
            rows.append((rc_written, (nx, ny), [_from_bits(w) for w in f[4:13]]))
        return rows
    return run


def _from_bits(word):
    return struct.unpack("<d", struct.pack("<Q", int(word, 16)))[0]


def all_cases():
    """(name, line): every case of this file, also what the sanitizer build of the program is run on"""
    cases = []
    for (name, (side, res0, off, res)), (k, centre) in itertools.product(LATTICES.items(), enumerate(CENTRES)):
        cases.append((f"same-{name}-{k}", walk_line(side, res0, centre, off, res, seed=k + 1)))
    # the caller's walk on half-cell boundaries of the search's grid, where the rounding decides: centres half a cell apart, either
    # sign, at small and large magnitude
    side, res0, off, res = LATTICES["61x61"]
    for k, centre in enumerate(CENTRES):
        for sx, sy in ((0.5, 0.5), (-0.5, 0.5), (1.5, -2.5)):
            w_centre = (centre[0] + sx * R, centre[1] + sy * R)
            cases.append((f"half-{k}-{sx}-{sy}", walk_line(side, res0, centre, off, res, w_centre=w_centre, w_offset=(0.1, 0.12), seed=10 + k)))
    # a caller geometry that is not the search's: other offsets, other resolutions (coarser and finer than the grid), other centre
    for k, centre in enumerate(CENTRES):
        cases.append((f"caller-{k}", walk_line(side, res0, centre, off, res, w_centre=(centre[0] + 0.01, centre[1] - 0.02), w_offset=(0.05, 0.1),
                                              w_res=(0.01, 0.0025), best_pose=(centre[0] + 0.02, centre[1] - 0.03, -0.2), seed=20 + k)))
        cases.append((f"caller-9x9-{k}", walk_line(9, R, centre, (2 * R, 1.5 * R), (R, 0.5 * R), w_offset=(1.5 * R, R), w_res=(0.5 * R, 0.25 * R), seed=30 + k)))
    return cases


def error_cases():
    side, res0, off, res = LATTICES["61x61"]
    cases = []
    for k, centre in enumerate(CENTRES):
        # the caller's offsets leave the side x side grid: in x only, in y only, in both, by one cell and by many
        for name, w_off in (("x", (0.155, 0.15)), ("y", (0.15, 0.155)), ("xy", (0.3, 0.3)), ("far", (40.0, 0.15))):
            cases.append((f"leave-{name}-{k}", walk_line(side, res0, centre, off, res, w_offset=w_off, seed=40 + k)))
        # the caller's centre a cell beside the grid: the first row or column is outside
        cases.append((f"shift-{k}", walk_line(side, res0, centre, off, res, w_centre=(centre[0] - R, centre[1]), seed=50 + k)))
        cases.append((f"shift-y-{k}", walk_line(side, res0, centre, off, res, w_centre=(centre[0], centre[1] + R), seed=50 + k)))
        # the search's own lattice does not fit the grid (a matcher whose search size is smaller): the first loop's error
        cases.append((f"small-{k}", walk_line(31, res0, centre, off, res, seed=60 + k)))
        cases.append((f"small-x-{k}", walk_line(5, R, centre, (3 * R, 2 * R), (R, R), seed=60 + k)))
    return cases


def test_separable_walk_equals_the_walk_as_written(check):
    cases = all_cases()
    rows = check([line for _, line in cases])
    ok = 0
    for (name, _), (rc, shape, cov) in zip(cases, rows):
        if name.startswith("same-"):
            assert shape == SHAPES[name.split("-")[1]], name
            assert rc == KH_OK, name
        ok += rc == KH_OK
        if rc == KH_OK:
            assert cov[1] == cov[3] and cov[0] > 0.0 and cov[4] > 0.0, name
    # the cases do what they are meant to do: most walks go through and reach the accumulation (a covariance off the identity)
    assert ok >= len(cases) * 3 // 4
    moved = [name for (name, _), (rc, _, cov) in zip(cases, rows) if rc == KH_OK and cov[0] != 1.0]
    assert len(moved) >= len(cases) // 2


def test_error_path(check):
    cases = error_cases()
    rows = check([line for _, line in cases])
    for (name, _), (rc, _, cov) in zip(cases, rows):
        assert rc == KH_ERR_SEARCH, name
        assert cov == [1.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 1.0], name        # SetToIdentity had run, nothing behind it


def test_response_below_tolerance(check):
    lines = []
    for (name, (side, res0, off, res)), centre in itertools.product(LATTICES.items(), CENTRES[:3]):
        for best in (0.0, 9.9e-7, -1.0):
            lines.append(walk_line(side, res0, centre, off, res, ang_res=0.02, best_response=best))
    # ... and in front of the error path: offsets that leave the grid are not looked at
    side, res0, off, res = LATTICES["61x61"]
    lines.append(walk_line(side, res0, CENTRES[1], off, res, w_offset=(0.3, 0.3), ang_res=0.02, best_response=0.0))
    for rc, _, cov in check(lines):
        assert rc == KH_OK
        assert cov == [MAX_VARIANCE, 0.0, 0.0, 0.0, MAX_VARIANCE, 0.0, 0.0, 0.0, 4 * (0.02 * 0.02)]
    # the first value at the tolerance takes the walk
    (rc, _, cov), = check([walk_line(side, res0, CENTRES[0], off, res, ang_res=0.02, best_response=1e-6)])
    assert rc == KH_OK and cov[0] not in (MAX_VARIANCE, 1.0) and cov[8] == 4 * (0.02 * 0.02)
