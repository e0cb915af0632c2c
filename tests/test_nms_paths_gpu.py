"""Every path of the NMS kernel (csrc/nms.hip) and of the candidate kernel
before it against oracle/yolo_ref.postprocess on the named cases of
tests/nms_cases.py: both sorters and both key stores on either side of their
boundaries, ties under each, the max_nms cut, the chunked greedy pass (chains
inside and across chunks, a kept list that every wave strides over), max_det
inside a chunk and at its end, the class filter after max_det, IoUs exactly
at the threshold, scale_boxes, the segmented layout with poisoned unused
slots, and one launch that mixes every kind of image.
test_nms_cases_cpu.py proves from the oracle alone that every case runs the
path it is named for.

No tolerances: boxes, scores, classes, order, out_n and cand_total are
compared bit for bit (every operation is f32 arithmetic the oracle restates),
and so are the candidate rows and segment counts of rv_candidates_from_raw.
The calls go through rvs_amd._lib on the test's own buffers: no engine, no
weights."""
import numpy as np
import pytest
import torch

import nms_cases as nm

pytestmark = pytest.mark.gpu
f32 = np.float32


@pytest.mark.parametrize("name", list(nm.cases()))
def test_case_vs_oracle(cuda, name):
    case = nm.cases()[name]
    dv = nm.device_run(case, cuda)
    if case.raw is not None:
        nm.compare_candidates(case, dv)
    else:
        assert dv.cand.tobytes() == case.cand.tobytes()  # the layout is only read
    nm.compare(case, dv)


def test_mixed_batch_images_alone(cuda):
    """Every image of the mixed launch gives the same bytes launched alone
    (as image 0: the workspace keys of the overflow images sit at b = 1 and
    b = 3 only in the batch), and two overflow images side by side."""
    case = nm.cases()["mixed_batch"]
    both = nm.device_run(case, cuda)
    nm.compare(case, both)
    for b in range(case.B):
        one = nm.device_run(case, cuda, images=[b])
        nm.compare(case, one, images=[b])
        assert one.out[0].tobytes() == both.out[b].tobytes()
        assert (one.out_n[0], one.cand_total[0]) == (both.out_n[b], both.cand_total[b])
    pair = nm.device_run(case, cuda, images=[3, 1])
    nm.compare(case, pair, images=[3, 1])


@pytest.mark.parametrize("key", list(nm.THRESHOLDS))
def test_kernel_compares_with_the_f32_it_is_given(cuda, key):
    """With the threshold rounded to the nearest f32 instead -- what the call
    site passed before it took the largest f32 not above the double -- the
    kernel is the oracle at that f32 threshold: at 0.6 and 0.3 the pair at the
    threshold stays (5 rows where the reference at the configured double has
    4), at 0.5 and 0.7 nothing changes."""
    case = nm.cases()[f"iou_at_{key}"]
    thr = nm.THRESHOLDS[key]
    near = float(f32(thr))
    dv = nm.device_run(case, cuda, iou_arg=near)
    ref = nm.postprocess(case, iou=near)
    for b in range(case.B):
        assert int(dv.out_n[b]) == len(ref[b]) == 5
        assert dv.out[b, :5].tobytes() == ref[b].tobytes()
        assert (len(nm.oracle(case.name).out[b]) == 4) == (key in ("0.6", "0.3"))


def test_argument_contract(cuda):
    from rvs_amd import _lib
    from rvs_amd._lib import RVError, call, ptr
    lib = _lib.load()
    B, cap, nseg = 2, 128, 2
    cand = torch.zeros((B, cap, 8), dtype=torch.float32, device=cuda)
    seg = torch.zeros((B, nseg), dtype=torch.int32, device=cuda)
    out = torch.zeros((B, 1024, 6), dtype=torch.float32, device=cuda)
    out_n = torch.full((B,), -1, dtype=torch.int32, device=cuda)
    sc = torch.tensor([1.0, 0, 0, 640, 640], dtype=torch.float32, device=cuda)
    assert lib.rv_nms_ws_bytes(B) == B * 65536 * 8 and lib.rv_nms_ws_bytes(0) == 0
    ws = torch.empty(lib.rv_nms_ws_bytes(B), dtype=torch.uint8, device=cuda)

    def nms(B=B, cap=cap, nseg=nseg, max_det=100, max_nms=30000, ws_bytes=ws.numel()):
        call("rv_nms_postprocess", ptr(cand), ptr(seg), B, cap, nseg, 0.7, max_det, max_nms,
             7680.0, ptr(sc), 0, ptr(out), ptr(out_n), 0, ptr(ws), ws_bytes, 0)

    nms()
    torch.cuda.synchronize()
    assert out_n.tolist() == [0, 0]
    for bad in [dict(max_det=0), dict(max_det=1025), dict(nseg=0), dict(nseg=1025, cap=65536),
                dict(nseg=3), dict(cap=65537), dict(cap=0), dict(max_nms=0),
                dict(ws_bytes=ws.numel() - 1)]:
        with pytest.raises(RVError):
            nms(**bad)
    out_n.fill_(-1)
    nms(B=0)
    torch.cuda.synchronize()
    assert out_n.tolist() == [-1, -1]  # B = 0: OK and nothing runs

    raw = torch.zeros((1, 5, 128), dtype=torch.float32, device=cuda)

    def cands(B=1, nc=1, A=128, cap=cap):
        call("rv_candidates_from_raw", ptr(raw), B, nc, A, 0.25, ptr(cand), cap, ptr(seg), 0)

    cands()
    for bad in [dict(A=65536, cap=65536), dict(A=129), dict(A=0), dict(nc=0)]:
        with pytest.raises(RVError):
            cands(**bad)
    cands(B=0)
    torch.cuda.synchronize()
    assert lib.rv_cand_segments(128) == 2 and lib.rv_cand_segments(129) == 3
