"""Seeded inputs for the tests of mcp_stereo_map_points' two host-checkable halves (mcptam_amd/csrc/stereo_append.h): created-point records for the
append, and stores for the busy gather.  Shared by tests/test_stereo_map_cpu.py and tests/test_stereo_map_gpu.py; tests/cpp/stereo_append_host_check.cpp
walks the same shapes under the sanitizers with a generator of its own."""
import numpy as np

from mcptam_amd import map_graph as mg
from mcptam_amd import stereo as S

BUSY_SIZES = (0, 1, 255, 256, 257)            # the workgroup seams of the gather (stereo.BUSY_BLOCK entries per workgroup)
assert S.BUSY_BLOCK == 256


def records(made, n_targets, level, seed):
    """`made` created-point records as k_stereo_walk leaves them: distinct candidates, root_pos = LevelZeroPos of a level position, every other
    double random (signed zeros and a subnormal among them: the append copies bits)."""
    rng = np.random.default_rng([seed, made, level])
    p = np.zeros(made, dtype=S.STEREO_POINT_DTYPE)
    p["candidate"] = rng.permutation(4 * made + 3)[:made]
    p["target"] = rng.integers(0, max(n_targets, 1), made)
    p["hypothesis"], p["score"] = rng.integers(0, 90, made), rng.integers(0, 5000, made)
    cxy = np.stack([rng.integers(0, 640 >> level, made), rng.integers(0, 480 >> level, made)], axis=1)
    p["root_pos"] = S.level_zero_pos(cxy, level)
    for f in ("world_pos", "target_pos", "center_nc", "one_right_nc", "one_down_nc", "pixel_right_w", "pixel_down_w"):
        p[f] = rng.normal(size=p[f].shape) * 10.0 ** rng.integers(-3, 4)
    if made:
        p["world_pos"][0, 0], p["pixel_down_w"][0, 2], p["target_pos"][made - 1, 1] = -0.0, 5e-324, 0.0
    return p, cxy.astype(np.int32)


def append_cases():
    """made in {0, 1, 7}; rows out of order and far apart; targets of one MKF slot and of several; levels 0 and 3; first_store 0 and not."""
    out = []
    for made in (0, 1, 7):
        for level, first_store, same_mkf in ((0, 0, True), (3, 4099, False), (0, 17, False), (3, 0, True)):
            n_targets = 3
            pts, cxy = records(made, n_targets, level, 11)
            rng = np.random.default_rng([made, level, first_store])
            rows = rng.permutation(np.concatenate([np.arange(5), [700, 123456, 2_000_000_000, 31, 65536]]))[:made + 2].astype(np.int32)      # two rows more than points
            out.append(dict(name="made%d_L%d_first%d_%s" % (made, level, first_store, "one_mkf" if same_mkf else "mkfs"), pts=pts, cxy=cxy, rows=rows, level=level,
                            src_mkf=5, src_cam=1, target_mkf=np.array([9, 9, 9] if same_mkf else [2, 9, 4095], dtype=np.int32),
                            target_cam=np.array([0, 1, 0], dtype=np.int32), first_store=first_store))
    return out


def store(n, src_mkf, src_cam, level, seed):
    """A store of n entries around the keyframe (src_mkf, src_cam): about half are its own (an eighth of those dead), the rest the same MKF under
    another camera, another MKF under the same camera, or neither; levels level-1 .. level+2 clipped to the pyramid; distinct positions, so the
    order of the gathered list is visible."""
    rng = np.random.default_rng([seed, n, src_mkf, src_cam])
    s = np.zeros(n, dtype=mg.STORE_ENTRY_DTYPE)
    kind = rng.integers(0, 8, n)
    s["mkf"] = np.where(kind < 6, src_mkf, src_mkf + 1 + rng.integers(0, 3, n))
    s["cam"] = np.where((kind < 4) | (kind == 6), src_cam, (src_cam + 1 + rng.integers(0, 2, n)) % 4)
    s["row"] = rng.permutation(max(n, 1) * 3)[:n]
    s["uv"] = np.arange(2 * n, dtype=np.float64).reshape(n, 2) * 0.25 - 3.0
    s["level"] = np.clip(level - 1 + rng.integers(0, 4, n), 0, 3)
    s["source"] = rng.integers(0, 5, n)
    s["alive"] = (rng.integers(0, 8, n) != 0).astype(np.int32)
    return s


def busy_cases():
    out = []
    for n in BUSY_SIZES:
        for level, src_mkf, src_cam in ((1, 3, 0), (2, 0, 1)):
            out.append(dict(name="n%d_L%d" % (n, level), store=store(n, src_mkf, src_cam, level, 7), src_mkf=src_mkf, src_cam=src_cam, level=level))
    full = store(256, 3, 0, 1, 9)                 # every entry of a whole workgroup matches
    full["mkf"], full["cam"], full["alive"] = 3, 0, 1
    out.append(dict(name="n256_all", store=full, src_mkf=3, src_cam=0, level=1))
    return out
