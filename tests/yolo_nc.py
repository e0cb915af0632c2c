"""Test-local helpers for YOLOv8 plans with a custom class count.

oracle/yolo_ref.conv_specs describes the 80-class model only.  conv_specs()
here gives the conv list for any class count by the Ultralytics Detect width
rule -- the class branch of every level is c3d = max(ch[0], min(nc, 100)) wide
(ch[0]: the P3 map's channels) and its last 1x1 conv maps c3d -> nc -- and
patched() swaps it in for the oracle (YoloRef, yolo_synth) at run time.
"""
import numpy as np

import yolo_synth
from oracle import yolo_ref

_SPECS80 = yolo_ref.conv_specs  # the oracle's own (80 classes), captured before any patch

REG = 16


def c3d_of(variant, nc):
    h15 = next(ci for n, ci, *_ in _SPECS80(variant)[0] if n == "model.22.cv3.0.0")
    return max(h15, min(nc, 100))


def conv_specs(variant, nc):
    """([(name, cin, cout, k, s, silu)], meta) of a YOLOv8 `variant` with `nc`
    classes, in state_dict order."""
    specs, meta = _SPECS80(variant)
    c3d = c3d_of(variant, nc)
    out = []
    for n, ci, co, k, s, act in specs:
        if n.startswith("model.22.cv3."):
            stage = n.rsplit(".", 1)[1]
            ci = ci if stage == "0" else c3d
            co = nc if stage == "2" else c3d
        out.append((n, ci, co, k, s, act))
    return out, meta


def patched(monkeypatch, nc):
    """The oracle and the synthetic-weight normaliser see `nc` classes: the
    patched conv list, and the road-class prior on the road ids below nc."""
    monkeypatch.setattr(yolo_ref, "conv_specs", lambda variant: conv_specs(variant, nc))
    road = tuple(c for c in yolo_synth.ROAD if c < nc)
    monkeypatch.setattr(yolo_synth, "ROAD", road)


def random_flat(variant, nc, seed=0):
    """Flat f32 weights of the state_dict shapes (plain seeded normals: for
    tests that only move values around)."""
    rng = np.random.default_rng(seed)
    parts = []
    for n, ci, co, k, s, act in conv_specs(variant, nc)[0]:
        parts += [rng.normal(0, 1 / np.sqrt(ci * k * k), co * ci * k * k), rng.normal(0, 0.05, co)]
    return np.concatenate(parts).astype(np.float32)


def split(variant, nc, flat):
    """(specs, {conv name: (weight (cout, cin, k, k), bias (cout,))}) views of flat."""
    specs, _ = conv_specs(variant, nc)
    params, off = {}, 0
    for n, ci, co, k, s, act in specs:
        nw = co * ci * k * k
        params[n] = (flat[off:off + nw].reshape(co, ci, k, k), flat[off + nw:off + nw + co])
        off += nw + co
    assert off == flat.size
    return specs, params
