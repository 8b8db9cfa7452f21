"""mcp_stereo_points: MapMakerServerBase::AddStereoMapPoints of one source keyframe and level in one call, against the composition in the shape
the shim had before it (one mcp_patch_sequences(EPI_COARSE) call per candidate and target, one EPI_REFINE call per candidate that survives the
selection), on the 640x480 and 1280x960 stereo scenes, levels 3 to 0, with 1, 3 and 5 targets.  Host-observed medians; the composition is
timed over the candidates the one call left alive for each target, its items packed beforehand, so only its calls and waits are counted.
Prints one JSON line.

Kernel times:  rocprofv3 --kernel-trace --stats -d /tmp/stereo_prof -o run -- python scripts/bench_stereo_points.py --quick
"""
import argparse
import ctypes
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np


def _med_ms(f, reps):
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        f()
        ts.append(time.perf_counter() - t0)
    return statistics.median(ts) * 1e3


PF_ITEM_DTYPE = None


def _composition(src, cam, pose_src, level, cand, targets, oc):
    """one call per (candidate, target) and per survivor, as the shim's EpipolarSearch / EpipolarRefine did; returns (runner, number of calls)"""
    from mcptam_amd import keyframe as K, stereo as S
    L = K.lib()
    global PF_ITEM_DTYPE
    if PF_ITEM_DTYPE is None:
        PF_ITEM_DTYPE = np.dtype([("point", S.TD_IN_DTYPE), ("point_key", "i4"), ("target", "i4"), ("start_pos", "f8", 2)], align=True)
        assert PF_ITEM_DTYPE.itemsize == ctypes.sizeof(K.PfItem)
    I = (np.eye(3), np.zeros(3))
    work = []
    for j, t in enumerate(targets):
        keep, _, tab, _, _, _ = K.marshal_patch_sequences([(t[0], t[1], t[2], I)], [[]], lambda k: k._h, lambda k: k._h)
        idx = np.nonzero(oc[j] != S.THINNED)[0]
        if len(idx) == 0:
            continue
        hyp, off = S.stereo_hypotheses(src, cam, pose_src, level, cand[idx], t)
        items = np.zeros(max(len(hyp), 1), dtype=PF_ITEM_DTYPE)
        items["point"][:len(hyp)] = hyp
        items["point_key"] = 1
        work.append((keep, tab, idx, off, items))
    n_calls = [0]

    def run():
        n = 0
        for keep, tab, idx, off, items in work:
            for q in range(len(idx)):
                cnt = int(off[q + 1] - off[q])
                st = K.new_pf_states(1)
                out = np.zeros(max(cnt, 1), dtype=K.TD_OUT_DTYPE)
                ss = np.array([0, cnt], dtype=np.int32)
                base = items.ctypes.data + int(off[q]) * PF_ITEM_DTYPE.itemsize
                L.mcp_patch_sequences(K.PF_EPI_COARSE, 1, tab, 1, ss.ctypes.data, base, st.ctypes.data, 3, 0, 0, out.ctypes.data)
                n += 1
                m = [(int(out[h]["score"]), h, out[h]["found_pos"].copy()) for h in np.nonzero(out["found"][:cnt])[0]]
                code, kept = S.select_matches(m)
                if code:
                    continue
                ref = np.zeros(len(kept), dtype=PF_ITEM_DTYPE)
                for k, mm in enumerate(kept):
                    ref[k] = items[int(off[q]) + mm[1]]
                    ref[k]["start_pos"] = mm[2]
                ss2 = np.array([0, len(kept)], dtype=np.int32)
                out2 = np.zeros(len(kept), dtype=K.TD_OUT_DTYPE)
                L.mcp_patch_sequences(K.PF_EPI_REFINE, 1, tab, 1, ss2.ctypes.data, ref.ctypes.data, st.ctypes.data, 3, 10, 0, out2.ctypes.data)
                n += 1
        n_calls[0] = n
    return run, n_calls


def main(quick=False, reps=10, comp_reps=3):
    from mcptam_amd import stereo as S, synth_img
    from mcptam_amd.keyframe import KeyFrame
    rows = []
    sizes = [(640, 480)] if quick else [(640, 480), (1280, 960)]
    for size in sizes:
        sc = synth_img.make_stereo_scene(size=size)
        src = KeyFrame(*size); src.MakeKeyFrame_Lite(sc["img_src"]); src.MakeKeyFrame_Rest()
        tgs = []
        for im in sc["imgs"]:
            g = KeyFrame(*size); g.MakeKeyFrame_Lite(im); tgs.append(g)
        cam = sc["cam"]
        for level in (3, 2, 1, 0):
            cand, _ = src.Candidates(level)
            for nt in ((3,) if quick else (1, 3, 5)):
                targets = [(tgs[j % 4], cam, sc["poses"][j % 4]) for j in range(nt)]
                got, keep, oc = S.stereo_points(src, cam, sc["pose_src"], level, cand, targets)
                one = _med_ms(lambda: S.stereo_points(src, cam, sc["pose_src"], level, cand, targets, outcomes=False), reps)
                run, n_calls = _composition(src, cam, sc["pose_src"], level, cand, targets, oc)
                comp = _med_ms(run, comp_reps)
                rows.append(dict(size="%dx%d" % size, level=level, targets=nt, candidates=int(len(cand)), created=int(len(got)), one_call_ms=round(one, 3),
                                 composition_ms=round(comp, 3), composition_calls=n_calls[0], speedup=round(comp / one, 1)))
                print("%-9s L%d %d targets: %5d cand, %4d points  one call %8.3f ms   composition %9.3f ms (%d calls)  x%.1f"
                      % (rows[-1]["size"], level, nt, len(cand), len(got), one, comp, n_calls[0], comp / one), file=sys.stderr)
    key = next((r for r in rows if r["size"] == "640x480" and r["level"] == 1 and r["targets"] == 3), None)
    print(json.dumps(dict(bench="stereo_points", rows=rows, headline=key)))


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--quick", action="store_true", help="640x480 only, 3 targets")
    a = ap.parse_args()
    main(quick=a.quick)
