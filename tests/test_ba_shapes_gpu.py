"""The linearisation, Schur and assembly kernels (csrc/ba_group.h, ba_schur4.h) at the seams of their group shapes, on the maps
of ba_shapes.py: every case first asserts through ChainBundle.DebugStructure() that the map took the path the case is named
for, then compares the reduced system (S per 6 x 6 block to 1e-10, rhs and J^T r to 1e-9 in the 2-norm) and the solution of the
damped normal equations (1e-7) with the oracle, and two independent builds bit for bit.

The oracle's results are computed once per map and never modified.  The tolerances are the project's (test_ba_gpu.py); the
oracle's own rounding floor on these maps is below 1e-12 (test_ba_shapes_cpu.py)."""
import numpy as np
import pytest

from ba_shapes import BATCH_LAMBDAS, POINT_SEAMS, POSE_SEAMS, block_scaled_error, get_map, rel_err_2
from helpers import rel_err

pytestmark = pytest.mark.gpu

TOL_S, TOL_RHS, TOL_X = 1e-10, 1e-9, 1e-7
LAYOUTS = ("small", "large")          # groups of 16 points (what a map of these sizes gets) / of 64 points (MCP_BA_SMALL_POINTS=0)
_ORACLE = {}


def _oracle(name, robust=True):
    """{'sys': {lambda: (S, rhs, b)}, 'x': (x_sparse, x_dense)} of the oracle on map `name`, computed once."""
    key = (name, robust)
    if key not in _ORACLE:
        from oracle import OracleBundle
        p = get_map(name)
        o = OracleBundle(p.cams, robust, True, False)
        p.populate(o)
        ref = {"sys": {lam: o.DebugSystem(lam) for lam in BATCH_LAMBDAS}}
        rc, xs, xd = o.DebugSolve(1.0)
        assert rc == 0
        ref["x"] = (xs, xd)
        for arrs in list(ref["sys"].values()) + [ref["x"]]:
            for a in arrs:
                a.setflags(write=False)
        _ORACLE[key] = ref
    return _ORACLE[key]


def _gpu(name, robust=True):
    from mcptam_amd.chain_bundle import ChainBundle
    p = get_map(name)
    g = ChainBundle(p.cams, robust, True, False)
    p.populate(g)
    return g


def _setup(monkeypatch, layout, **env):
    from mcptam_amd import chain_bundle
    chain_bundle.struct_cache_clear()
    if layout == "large":
        monkeypatch.setenv("MCP_BA_SMALL_POINTS", "0")
    for k, v in env.items():
        monkeypatch.setenv(k, v)


def _assert_system(got, ref, what):
    (Sg, rg, bg), (So, ro, bo) = got, ref
    assert Sg.shape == So.shape
    eS, er, eb = block_scaled_error(Sg, So), rel_err_2(rg, ro), rel_err_2(bg, bo)
    print("%s: S %.2e  rhs %.2e  b %.2e" % (what, eS, er, eb))
    assert eS <= TOL_S, (what, eS)
    assert er < TOL_RHS and eb < TOL_RHS, (what, er, eb)


def _bit_differences(a, b):
    """(entries that differ, largest difference relative to the largest entry) between two (S, rhs, b) triples"""
    n = sum(int((x != y).sum()) for x, y in zip(a, b))
    d = max(float(np.abs(x - y).max() / max(np.abs(x).max(), 1e-300)) for x, y in zip(a, b))
    return n, d


def _check(name, expect, robust=True):
    """The full comparison of one map under the environment in effect; `expect`: DebugStructure() entries that make the case
    mean something (a callable value is a predicate).  Returns the report."""
    ref = _oracle(name, robust)
    outs = []
    for rep in range(2):
        g = _gpu(name, robust)
        if rep == 0:
            st = g.DebugStructure()
            print(name, st)
            for k, v in expect.items():
                assert (v(st[k]) if callable(v) else st[k] == v), (name, k, st[k], st)
        outs.append(g.DebugSystem(1e-2))
        if rep == 0:
            xs, xd = ref["x"]
            assert rel_err(xs, xd) < TOL_X                         # the oracle's own two solvers agree: the map is well enough conditioned
            xg = g.DebugSolve(1.0)
            assert xg.shape == xs.shape
            ex = rel_err(xg, xs)
            print("%s: x %.2e" % (name, ex))
            assert ex < TOL_X, (name, ex)
        g.close()
    _assert_system(outs[0], ref["sys"][1e-2], name)
    _assert_system(outs[1], ref["sys"][1e-2], name + " (second build)")
    ndiff, rdiff = _bit_differences(outs[0], outs[1])
    print("%s: two builds differ in %d entries, by %.2e of the largest" % (name, ndiff, rdiff))
    assert ndiff == 0, (name, ndiff, rdiff)
    return st


def _ngroups(n, per):
    return (n + per - 1) // per


# ---------------------------------------------------------------------------------------------------------------------
# the multi-chunk runs of k_schur_group come first: they had never run under a test

def _large_maps():
    return (["pts%d" % n for n in POINT_SEAMS] + ["shared%d_130" % k for k in POSE_SEAMS] + ["roll5", "roll13", "big_all", "big_mixed", "big_one",
            "meas", "meas_plain", "tencam", "calib17", "calib65"])


@pytest.mark.parametrize("name", _large_maps())
def test_schur_group_kernel_on_every_map_of_the_large_layout(gpu_required, name, monkeypatch):
    """MCP_BA_SCHUR4=0: k_schur_group with groups of up to 64 points -- up to four 16-point chunks per group, with the index
    prologue over all chunks, the prefetch one chunk ahead and the clearing of the rows a chunk wrote."""
    # (groups are closed at 13 poses by default, which leaves every point that sees 14 to 16 poses alone in its group:
    #  MCP_BA_GROUP_LMAX13=0 fills groups to 16 poses -- four chunks with all 96 rows of the local tile in use)
    _setup(monkeypatch, "large", MCP_BA_SCHUR4="0", **({"MCP_BA_GROUP_LMAX13": "0"} if name in ("shared14_130", "shared16_130") else {}))
    robust = name != "meas_plain"
    name = "meas" if name == "meas_plain" else name
    p = get_map(name)
    expect = dict(grp_pts=64, schur_kernel="schur_group")
    if name.startswith("pts") or name.startswith("shared"):
        n = p.n_points
        expect.update(ngroup=_ngroups(n, 64), grp_points_max=min(n, 64), grp_points_min=(n - 1) % 64 + 1, nbig=0)
    st = _check(name, expect, robust)
    if name in ("pts17", "pts63", "pts64", "pts65", "pts129", "shared16_130", "shared14_130", "shared13_130", "meas", "calib65"):
        assert st["grp_points_max"] > 16, st          # a multi-chunk group


# ---------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("n", POINT_SEAMS)
def test_point_count_seams(gpu_required, n, layout, monkeypatch):
    """All points share six free poses: groups close on the point count alone -- a last group of 1, 15, 16, 17 (1 beyond a quad
    group / a chunk), 63, 64, 65 and 129 (1 beyond one and two full groups) points."""
    _setup(monkeypatch, layout)
    per = 16 if layout == "small" else 64
    _check("pts%d" % n, dict(grp_pts=per, ngroup=_ngroups(n, per), grp_points_max=min(n, per), grp_points_min=(n - 1) % per + 1,
                             grp_poses_max=6, nbig=0, grp_no_pose=0, schur_kernel="schur4", lin_generic=False,
                             lin_kernel="quad" if layout == "small" else "pipe", nfl=n, np=36))


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("k,fill16", [(k, False) for k in POSE_SEAMS] + [(14, True), (16, True)])
@pytest.mark.parametrize("asm_long", [None, "0", "1"])
def test_pose_count_seams_shared_set(gpu_required, k, fill16, layout, asm_long, monkeypatch):
    """All points see the same k free poses: 13 fills k_schur4's local tile (rows 78 and 79 of 80 unused, the guards la < 13),
    14 and 16 fall to k_schur_group.  Groups are closed at 13 poses, so a point that sees 14 or 16 is alone in its group (as many
    groups as points); fill16 (MCP_BA_GROUP_LMAX13=0) fills the groups to 16 poses: full groups of 14 and 16 poses, and 16 poses in
    groups of 16 points no longer fit the quad kernel's LDS and take k_linearize_pipe with 16-point groups.  asm_long: the same
    through k_assemble_long (1) and k_assemble (0) by force."""
    env = {} if asm_long is None else {"MCP_BA_ASM_LONG": asm_long}
    if fill16:
        env["MCP_BA_GROUP_LMAX13"] = "0"
    _setup(monkeypatch, layout, **env)
    n, per = (66, 16) if layout == "small" else (130, 64)
    expect = dict(grp_pts=per, grp_poses_max=k, nbig=0, grp_no_pose=0, schur_kernel="schur4" if k <= 13 and not fill16 else "schur_group",
                  lin_generic=False, np=6 * k, nfl=n)
    if k <= 13 or fill16:
        expect.update(ngroup=_ngroups(n, per), grp_points_max=per, grp_points_min=(n - 1) % per + 1)
    else:
        expect.update(ngroup=n, grp_points_max=1, grp_points_min=1)
    if layout == "large":
        expect["lin_kernel"] = "pipe"
    elif k == 16 and fill16:
        expect["lin_kernel"] = "pipe"                  # 136 pose blocks + 256 W blocks: 76 KB, the quad form does not fit
    elif k <= 13 or not fill16:
        expect["lin_kernel"] = "quad"
    if asm_long is not None:
        expect["asm_long"] = asm_long == "1"
    _check("shared%d_%d" % (k, n), expect)


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("lmax13", [True, False])
@pytest.mark.parametrize("k", [5, 13])
def test_pose_count_seams_rolling_sets(gpu_required, k, lmax13, layout, monkeypatch):
    """Point i sees poses {i, ..., i + k - 1} (mod 66): groups close on the pose budget -- at exactly 13 poses for k_schur4,
    at 16 (MCP_BA_GROUP_LMAX13=0) for k_schur_group."""
    _setup(monkeypatch, layout, **({} if lmax13 else {"MCP_BA_GROUP_LMAX13": "0"}))
    st = _check("roll%d" % k, dict(grp_poses_max=13 if lmax13 else 16, schur_kernel="schur4" if lmax13 else "schur_group",
                                   ngroup=lambda v: v > 1, nbig=0, np=6 * 66, nfl=66, lin_generic=False))
    assert st["grp_points_max"] < st["grp_pts"], st          # closed by the poses, not by the point count


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("name,nbig", [("big_all", 20), ("big_mixed", 20), ("big_one", 1)])
def test_points_seen_from_more_poses_than_a_group_holds(gpu_required, name, nbig, layout, monkeypatch):
    """17 free poses per point: the generic path (k_linearize, k_schur) -- for every point of the map (groups without a pose),
    for every other point, for one point riding in a normal group."""
    _setup(monkeypatch, layout)
    expect = dict(nbig=nbig, lin_generic=True, np=6 * 17, grp_poses_max=0 if name == "big_all" else 6)
    st = _check(name, expect)
    if name == "big_all":
        assert st["grp_no_pose"] == st["ngroup"] >= 1, st
    else:
        assert st["grp_no_pose"] < st["ngroup"], st


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("name", ["big_all", "big_mixed", "big_one"])
def test_two_builds_of_a_map_with_generic_path_points_give_the_same_bytes(gpu_required, name, layout, monkeypatch):
    """Two independent builds of the reduced system are the same bytes also when points go through the generic path.

    k_linearize and k_schur (csrc/ba_kernels.h) serve the points that see more than 16 free poses.  They used to add into U, J^T r,
    V, g, W and S with global fp64 atomics from many workgroups, in the order the wavefronts arrived: of the 102 x 102 + 2 x 102
    numbers, two builds of big_all differed in 1800 to 3100, of big_mixed in 2600 to 3500, of big_one in 0 to 4100, by 2e-16 to 2.3e-15
    of the largest entry.  Now one wavefront (linearisation) and one workgroup per system (elimination) take those points in a fixed
    order."""
    _setup(monkeypatch, layout)
    outs = []
    for _ in range(2):
        g = _gpu(name)
        assert g.DebugStructure()["lin_generic"]
        outs.append(g.DebugSystem(1e-2))
        g.close()
    ndiff, rdiff = _bit_differences(outs[0], outs[1])
    print("%s: two builds differ in %d entries, by %.2e of the largest" % (name, ndiff, rdiff))
    assert ndiff == 0, (name, ndiff, rdiff)


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("robust", [True, False])
def test_measurement_count_seams(gpu_required, robust, layout, monkeypatch):
    """1, 2, 3, 4, 5, 7, 8 and 9 measurements per point (the quad kernel deals them to four lanes, the pipe kernel runs one round
    ahead) for points expressed in the fixed and in a free keyframe, points whose only observer is their own source pose, free
    points seen only from the fixed keyframe, fixed points seen from free poses and from the fixed one only."""
    _setup(monkeypatch, layout)
    _check("meas", dict(grp_pts=16 if layout == "small" else 64, nbig=0, np=36, nfl=64, schur_kernel="schur4",
                        lin_kernel="quad" if layout == "small" else "pipe"), robust)


@pytest.mark.parametrize("layout", LAYOUTS)
def test_ten_camera_rig(gpu_required, layout, monkeypatch):
    """Cameras 8 and 9 do not live in the linearisation kernels' LDS table (LIN_LDS_CAMS = 8): read from global memory."""
    _setup(monkeypatch, layout)
    _check("tencam", dict(grp_pts=16 if layout == "small" else 64, nbig=0, np=36, lin_kernel="quad" if layout == "small" else "pipe",
                          schur_kernel="schur4"))


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("n", [17, 65])
def test_calibration_shape_at_a_seam(gpu_required, n, layout, monkeypatch):
    """One pose vertex at two positions of an edge (the calibration's relative camera poses), cut to one point beyond a group."""
    _setup(monkeypatch, layout)
    _check("calib%d" % n, dict(grp_pts=16 if layout == "small" else 64, nbig=0, lin_kernel="quad" if layout == "small" else "pipe",
                               schur_kernel="schur4"))


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("nsys", [2, 3, 4])
@pytest.mark.parametrize("k", [13, 16])
def test_batched_systems(gpu_required, k, nsys, layout, monkeypatch):
    """Systems 1 to 3 of a batch (k_schur4: wavefront q is system q; k_schur_group: blockIdx.y = q): each agrees with the oracle at
    its own lambda and is, bit for bit, the single system a fresh handle builds for that lambda."""
    _setup(monkeypatch, layout, **({"MCP_BA_GROUP_LMAX13": "0"} if k == 16 else {}))          # (16 poses: full groups, see above)
    name = "shared%d_%d" % (k, 66 if layout == "small" else 130)
    ref = _oracle(name)
    lams = BATCH_LAMBDAS[:nsys]
    g = _gpu(name)
    st = g.DebugStructure()
    assert st["schur_kernel"] == ("schur4" if k == 13 else "schur_group") and st["max_systems"] >= nsys and st["grp_poses_max"] == k, st
    assert st["grp_points_max"] == st["grp_pts"], st
    batch = g.DebugSystems(lams)
    with pytest.raises(RuntimeError, match="buffers for"):
        g.DebugSystems(list(BATCH_LAMBDAS) + [1e3])
    g.close()
    assert len(batch) == nsys
    for q, lam in enumerate(lams):
        _assert_system(batch[q], ref["sys"][lam], "%s system %d of %d" % (name, q, nsys))
        f = _gpu(name)
        single = f.DebugSystem(lam)
        f.close()
        for a, b in zip(batch[q], single):
            assert np.array_equal(a, b), (name, q, lam)
