"""Sparse Detect head (RV_YOLO_OPT_HEAD_SPARSE; csrc/head_box.hip) against
the dense head: the class-only decode + the per-candidate box branch must
give the candidate segments of the dense convs + full decode bit for bit --
counts, boxes, scores, classes, anchors and order (rows compared as int32
bit patterns).  Each form is forced through the option; rv_yolo_head_form
proves which kernels ran (2 dense, 3 sparse).

Shapes: 96x160 is the smallest frame with all three levels non-trivial (P3
12x20, P4 6x10, P5 3x5: every P5 anchor has neighbours outside the map);
at conf 0 all 315 anchors of an image are candidates, so every corner and
edge of every level, full 16-candidate groups and a ragged last group are
covered.  1080p at the production conf is the working regime: sparse lists,
empty segments, partly filled groups."""
import numpy as np
import pytest
import torch

from conftest import road_frame
from oracle import cpu, yolo_ref

pytestmark = pytest.mark.gpu

SMALL = (96, 160)
DENSE, SPARSE = 0, 1


def _frames(H, W, B, seed=30):
    return np.stack([cpu.median(cpu.clahe_ycrcb(road_frame(H, W, seed=seed + b)), 3)
                     for b in range(B)])


def _engine(cuda, H, W, B, variant=0, conf=0.25):
    from rvs_amd.detect import weights
    from rvs_amd.detect.yolo_hip import YoloEngine
    flat = weights.synthetic_weights(variant, seed=1)
    eng = YoloEngine(variant, flat, B, (H, W), imgsz=max(H, W), conf=conf, device=cuda)
    return eng


def _forward(eng, lb, mode):
    """One forward with the head form forced: (head form, counts (B, nseg),
    rows (B, cap, 8) int32).  The candidate buffers start as NaN / -7, so a
    row or count the forward left unwritten cannot compare equal by luck."""
    B = lb.shape[0]
    eng.set_head_sparse(mode)
    eng.cand[0].fill_(float("nan"))
    eng.seg_n[0].fill_(-7)
    eng.forward_raw(lb)
    torch.cuda.synchronize()
    seg = eng.seg_n[0].view(-1)[:B * eng.nseg].view(B, eng.nseg).cpu().numpy().copy()
    return eng.head_form(), seg, eng.cand[0][:B].cpu().numpy().view(np.int32).copy()


def _assert_same(dense, sparse):
    (fd, sd, rd), (fs, ss, rs) = dense, sparse
    assert (fd, fs) == (2, 3)
    assert (sd >= 0).all() and (sd <= 64).all()
    np.testing.assert_array_equal(sd, ss)
    for b in range(sd.shape[0]):
        for j in np.nonzero(sd[b])[0]:
            k = int(sd[b, j])
            np.testing.assert_array_equal(rd[b, 64 * j:64 * j + k], rs[b, 64 * j:64 * j + k],
                                          err_msg=f"image {b} segment {j}")
    return int(sd.sum())


def _trace(eng):
    from rvs_amd import _lib
    lib = _lib.load()
    n = lib.rv_yolo_trace(eng._h, None, 0)
    recs = np.zeros(n * 24, np.int32)
    lib.rv_yolo_trace(eng._h, recs.ctypes.data, n)
    return recs.reshape(n, 24)


def _launches_without_config(eng):
    """(indices of the last forward's launches that have no conv
    configuration, number of launches)."""
    from rvs_amd import _lib
    lib, out, idx = _lib.load(), [], 0
    while True:
        c = lib.rv_yolo_conv_candidates(eng._h, idx, None, 0)
        if c < 0:
            return out, idx
        if c == 0:
            out.append(idx)
        idx += 1


def test_every_border_case(cuda):
    H, W = SMALL
    B = 3
    eng = _engine(cuda, H, W, B, conf=0.0)
    assert (eng.in_h, eng.in_w) == SMALL and eng.A == 315
    lb = eng.letterbox(torch.from_numpy(_frames(H, W, B)).to(cuda))
    dense = _forward(eng, lb, DENSE)
    sparse = _forward(eng, lb, SPARSE)
    assert _assert_same(dense, sparse) == B * 315  # every anchor a candidate
    eng.close()


def test_working_regime(cuda):
    H, W, B = 1080, 1920, 2
    from rvs_amd.detect import weights
    from rvs_amd.detect.yolo_hip import YoloEngine
    eng = YoloEngine(0, weights.synthetic_weights(0, seed=0), B, (H, W), device=cuda)
    assert eng.conf == 0.25
    lb = eng.letterbox(torch.from_numpy(_frames(H, W, B, seed=7)).to(cuda))
    dense = _forward(eng, lb, DENSE)
    tr_dense = _trace(eng)
    none_dense, n_dense = _launches_without_config(eng)
    sparse = _forward(eng, lb, SPARSE)
    tr_sparse = _trace(eng)
    none_sparse, n_sparse = _launches_without_config(eng)
    total = _assert_same(dense, sparse)
    seg = dense[1]
    print(f"{total} candidates of {B * eng.A} anchors; {(seg == 0).sum()} of {seg.size} segments empty")
    assert 0 < total < 0.2 * B * eng.A and (seg == 0).any() and ((seg % 16) != 0).any()
    # trace: the same conv list; exactly the cv2.i.1 convs carry the mark
    # "no output map" (out0.buf = -1) in the sparse forward, none in the dense
    names = [s[0] for s in yolo_ref.conv_specs(0)[0]]
    np.testing.assert_array_equal(tr_dense[:, 0], tr_sparse[:, 0])
    assert (tr_dense[:, 8] >= 0).all()
    marked = sorted(names[i] for i in tr_sparse[tr_sparse[:, 8] < 0, 0])
    assert marked == [f"model.22.cv2.{i}.1" for i in range(3)]
    # launch list: the same length (the skipped convs keep their index as
    # placeholders that cannot be launched), three more entries without a
    # configuration than the dense list
    assert n_sparse == n_dense and len(none_sparse) == len(none_dense) + 3
    assert set(none_dense) <= set(none_sparse)
    eng.close()


def test_no_candidates(cuda):
    """conf 0.9999 with the shipped calibration at the shape it was made for
    (1080p: the best class score stays below 0.5; at the small shape the
    same weights saturate past 0.9999), one image all zeros: zero counts
    everywhere, the sparse kernel finds nothing to do."""
    H, W, B = 1080, 1920, 2
    from rvs_amd.detect import weights
    from rvs_amd.detect.yolo_hip import YoloEngine
    eng = YoloEngine(0, weights.synthetic_weights(0, seed=0), B, (H, W), conf=0.9999, device=cuda)
    fr = _frames(H, W, B, seed=7)
    fr[1] = 0
    lb = eng.letterbox(torch.from_numpy(fr).to(cuda))
    dense = _forward(eng, lb, DENSE)
    sparse = _forward(eng, lb, SPARSE)
    assert _assert_same(dense, sparse) == 0
    assert (sparse[1] == 0).all()
    eng.close()


def test_option_round_trip_with_tuned_configs(cuda):
    H, W = SMALL
    B = 3
    eng = _engine(cuda, H, W, B)
    lb = eng.letterbox(torch.from_numpy(_frames(H, W, B)).to(cuda))
    eng.set_head_sparse(DENSE)
    assert eng.autotune(lb, reps=1) == 0
    cfgs = eng.tuned_configs()
    assert len(cfgs) > 0 and any(c[0] > 0 for c in cfgs)
    eng.load_tuned(cfgs)
    d0 = _forward(eng, lb, DENSE)
    s = _forward(eng, lb, SPARSE)
    d1 = _forward(eng, lb, DENSE)
    assert _assert_same(d0, s) > 0
    _assert_same(d1, s)
    assert eng.tuned_configs() == cfgs
    # auto (the default): dense for this small batch, whatever conf
    assert _forward(eng, lb, "auto")[0] == 2
    eng.close()


def test_auto_picks_sparse_for_pipeline_batches(cuda):
    H, W = SMALL
    B = 8
    eng = _engine(cuda, H, W, B)
    lb = eng.letterbox(torch.from_numpy(_frames(H, W, B)).to(cuda))
    dense = _forward(eng, lb, DENSE)
    auto = _forward(eng, lb, "auto")
    assert _assert_same(dense, auto) > 0
    eng.conf = 0.0  # every anchor a candidate: auto stays dense
    assert _forward(eng, lb, "auto")[0] == 2
    eng.close()


def test_yolov8s_option_keeps_dense_results(cuda):
    """YOLOv8s' class branch is 128 wide, so its decode is not the fixed form
    and the sparse option does not apply: forwards stay dense (form 1) and
    equal under either setting."""
    import yolo_synth
    from rvs_amd.detect.yolo_hip import YoloEngine
    H, W = SMALL
    B = 3
    flat, fr = yolo_synth.synth_case(1, H, W, B, max(H, W))
    eng = YoloEngine(1, flat, B, (H, W), imgsz=max(H, W), device=cuda)
    lb = eng.letterbox(torch.from_numpy(fr.copy()).to(cuda))
    (fd, sd, rd), (fs, ss, rs) = _forward(eng, lb, DENSE), _forward(eng, lb, SPARSE)
    assert (fd, fs) == (1, 1) and sd.sum() > 0
    np.testing.assert_array_equal(sd, ss)
    for b in range(B):
        for j in np.nonzero(sd[b])[0]:
            k = int(sd[b, j])
            np.testing.assert_array_equal(rd[b, 64 * j:64 * j + k], rs[b, 64 * j:64 * j + k])
    eng.close()
