"""The seeded map of the re-find tests (tests/test_refind_cpu.py, tests/test_refind_gpu.py), and the composition mcp_map_refind is checked
against: mcp_patch_sequences(MCP_PF_REFIND, range 4) -- or the CPU oracle's restatement of it -- on items packed from the same columns, with
the sequences the map maker's ReFindBatch builds, then mcptam_amd.refind.refind_verdicts.

The map: make_tracking_scene(); source keyframe A (MakeKeyFrame_Lite + MakeKeyFrame_Rest of view A); rows 0..935 are the 936 points of
make_map_points; rows 936..5999 are entries 936.. of make_map_cloud(base, 6000, seed=1, spread=30.0) with level = default_rng(9).integers(0, 4,
6000) and source centres drawn next from the same generator, uniformly over the whole level image (border included: bad templates).  Against
view B at poseB the CPU oracle gives OUTSIDE 3859, TEMPLATE_BAD 190, NOT_FOUND 1230, FOUND 721 (293 at level 0, 428 above)."""
import numpy as np

N_ROWS = 6000
N_BASE = 936
EXPECTED = {2: 3859, 3: 190, 4: 1230, 1: 721}      # verdict -> pairs, against B
EXPECTED_FOUND_L0, EXPECTED_FOUND_UP = 293, 428
IDENT = (np.eye(3), np.zeros(3))


def make_world(kf_class, oracle_class=None):
    """kf_class: the keyframe type the columns' sources are (mcptam_amd.keyframe.KeyFrame on the GPU, oracle.OracleKeyFrame on the CPU);
    oracle_class: additionally build the oracle's twins (A_o, B_o) for the oracle comparison."""
    from mcptam_amd import synth_img
    sc = synth_img.make_tracking_scene()
    A = kf_class(640, 480)
    A.MakeKeyFrame_Lite(sc["imgA"]); A.MakeKeyFrame_Rest()
    B = kf_class(640, 480)
    B.MakeKeyFrame_Lite(sc["imgB"])
    base = synth_img.make_map_points(sc["cam"], A, None, sc["poseA"], sc["depth"])
    assert len(base) == N_BASE
    bw, bp, bd = synth_img.points_soa(base)
    cw, cp, cd, cu = synth_img.make_map_cloud(base, N_ROWS, seed=1, spread=30.0)
    rng = np.random.default_rng(9)
    level = rng.integers(0, 4, N_ROWS)
    cx = rng.integers(0, 640 >> level)
    cy = rng.integers(0, 480 >> level)
    k = N_BASE
    cols = dict(wp=np.concatenate([bw, cw[k:]]), pr=np.concatenate([bp, cp[k:]]), pd=np.concatenate([bd, cd[k:]]),
                usable=np.concatenate([np.ones(k, dtype=np.uint8), cu[k:]]), keys=np.arange(N_ROWS, dtype=np.int32) * 3 + 7,
                level=np.concatenate([[p["source_level"] for p in base], level[k:]]).astype(np.int32),
                center=np.ascontiguousarray(np.concatenate([[p["center"] for p in base], np.stack([cx, cy], axis=1)[k:]]).astype(np.int32)),
                fixed=np.zeros(N_ROWS, dtype=np.uint8))
    w = dict(sc=sc, cam=sc["cam"], A=A, B=B, cols=cols, n=N_ROWS, base=base)
    if oracle_class is not None:
        Ao = oracle_class(640, 480)
        Ao.MakeKeyFrame_Lite(sc["imgA"]); Ao.MakeKeyFrame_Rest()
        Bo = oracle_class(640, 480)
        Bo.MakeKeyFrame_Lite(sc["imgB"])
        w.update(A_o=Ao, B_o=Bo)
    return w


def moved(pose, w3, dt):
    """pose turned by exp(w3) and shifted by dt (CamFromWorld)."""
    from mcptam_amd.synth import so3_exp
    R, t = pose
    return so3_exp(np.asarray(w3, dtype=np.float64)) @ R, t + np.asarray(dt, dtype=np.float64)


def newly_made_targets(sc, kf):
    """The four views of the ReFindNewlyMade shape: B; B moved a little (shares templates); turned by pi (sees nothing); turned by 0.25 rad."""
    pB = sc["poseB"]
    return [(kf, sc["cam"], pB), (kf, sc["cam"], moved(pB, (0.0003, -0.0002, 0.001), (0.003, -0.001, 0.002))),
            (kf, sc["cam"], moved(pB, (0.0, np.pi, 0.0), (0.0, 0.0, 0.0))), (kf, sc["cam"], moved(pB, (0.0, 0.25, 0.0), (0.0, 0.0, 0.0)))]


def sequences_of(pairs, per_row_finders):
    """Start index of every sequence, as ReFindBatch cuts them: every pair alone, or maximal runs of one row."""
    pairs = np.asarray(pairs).reshape(-1, 2)
    n = len(pairs)
    if n == 0:
        return np.zeros(0, dtype=np.int64)
    head = np.ones(n, dtype=bool)
    if per_row_finders:
        head[1:] = pairs[1:, 0] != pairs[:-1, 0]
    return np.nonzero(head)[0]


def compose(cols, src, targets, pairs, per_row_finders=False, finder=None, search=None, src_oracle=None):
    """The composition.  src: the source keyframe of every row (one object, or a list per row); targets: list of (keyframe, camera, CamFromWorld);
    search: mcptam_amd.keyframe.patch_sequences (default) or oracle.oracle_patch_sequences (then src_oracle names the oracle's source and the
    targets hold oracle keyframes).  finder: PF_STATE_DTYPE array of one element or None.
    Returns (verdicts, measurements, counts, finder state after the last sequence (1,), td_out records)."""
    from mcptam_amd import keyframe as K
    from mcptam_amd.refind import refind_verdicts, verdict_counts
    if search is None:
        search = K.patch_sequences
    pairs = np.asarray(pairs, dtype=np.int32).reshape(-1, 2)
    starts = sequences_of(pairs, per_row_finders)
    ends = np.concatenate([starts[1:], [len(pairs)]])

    def point(r):
        s = src[r] if isinstance(src, list) else src
        return dict(world_pos=cols["wp"][r], pixel_right_w=cols["pr"][r], pixel_down_w=cols["pd"][r], source_kf=s, source_kf_oracle=src_oracle,
                    source_level=int(cols["level"][r]), center=(int(cols["center"][r][0]), int(cols["center"][r][1])), fixed=int(cols["fixed"][r]))
    seqs = [[dict(point=point(int(pairs[i, 0])), point_key=int(cols["keys"][pairs[i, 0]]), target=int(pairs[i, 1])) for i in range(a, b)]
            for a, b in zip(starts, ends)]
    states = K.new_pf_states(len(seqs))
    if finder is not None and len(seqs):
        states[0] = finder[0]
    out = search(K.PF_REFIND, [(kf, cam, pose, IDENT) for kf, cam, pose in targets], seqs, states, 4, 8)
    v, m = refind_verdicts(out, pairs)
    last = states[-1:].copy() if len(seqs) else (K.new_pf_states(1) if finder is None else finder.copy())
    return v, m, verdict_counts(v), last, out


def same_meas(a, b, pos_tol=0.0):
    """Field by field; positions bit for bit (pos_tol = 0) or within pos_tol."""
    if len(a) != len(b):
        return False
    for f in ("pair", "row", "target", "level", "subpix", "score"):
        if not np.array_equal(a[f], b[f]):
            return False
    if pos_tol == 0.0:
        return np.array_equal(a["root_pos"], b["root_pos"])
    return bool(len(a) == 0 or np.abs(a["root_pos"] - b["root_pos"]).max() <= pos_tol)


def same_state(a, b):
    return all(np.array_equal(a[f], b[f], equal_nan=a[f].dtype.kind == "f") for f in a.dtype.names)
