"""Recorder of the C-ABI calls a forward makes, and the cases whose records ``tests/golden/launch_records.json`` keeps.

``libgw_amd.so`` computes; the Python layer only decides which of its entry points run, in which order, on which operands and
streams.  Two trees that make the same calls therefore compute the same thing, and a refactor of the Python layer is checked
by comparing call records: every Python caller fetches the library through ``_lib.lib()``, which returns the module global
``_lib._lib`` - a proxy put there notes each call and passes it through.

Per call the record holds the entry name and, per argument: integers and floats by value; a pointer as 0 (null) / 1; a struct
(``GwOperand``, ``GwMlpWeights``, the save struct, ...) as the list of its fields under the same rules; an array as the list of
its elements; the stream (last parameter of every launching entry, include/gw_amd.h) as the ordinal of its first appearance in
the record.  No address is ever recorded.  ``gw_version`` and ``gw_last_error`` are skipped.

``python -m tests.launch_record OUT.json`` writes the golden (on the commit whose behaviour is to be kept); the GPU test
``tests/test_gpu_launch_record.py`` compares.  Each case is a cold call followed by a warm call of one freshly built model.
The file stores each distinct call once (``calls``) and a case as a list of indices into that table."""
from __future__ import annotations

import contextlib
import ctypes
import json
import os
import re
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import graph_weather_amd as gw  # noqa: E402
from graph_weather_amd import _lib, ops  # noqa: E402
from graph_weather_amd.layers import set_compute_dtype, set_deterministic  # noqa: E402
from graph_weather_amd.utils import deterministic_fill_, regular_lat_lons, seeded_features  # noqa: E402

DEV = "cuda:0"
GOLDEN = os.path.join(ROOT, "tests", "golden", "launch_records.json")
SKIP = ("gw_version", "gw_last_error")
_INT_TYPES = (ctypes.c_int, ctypes.c_int32, ctypes.c_int64, ctypes.c_uint32, ctypes.c_size_t, ctypes.c_long, ctypes.c_ulong)
_FLOAT_TYPES = (ctypes.c_float, ctypes.c_double)


def _entries_with_stream():
    """Names of the entry points whose last parameter is ``void* stream`` (the ABI's convention), read from the header."""
    text = open(os.path.join(ROOT, "include", "gw_amd.h")).read()
    text = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
    return {m.group(1) for m in re.finditer(r"\b(gw_\w+)\s*\(([^;{}]*?)\)\s*;", text) if re.search(r"void\s*\*\s*stream\s*$", m.group(2))}


def _value(v):
    """A ctypes field / element / by-pointer argument without its addresses."""
    if v is None:
        return 0
    if isinstance(v, ctypes.Structure):
        return [int(bool(getattr(v, f[0]))) if f[1] in (ctypes.c_void_p, ctypes.c_char_p) else _value(getattr(v, f[0]))
                for f in v._fields_]
    if isinstance(v, ctypes.Array):
        if issubclass(v._type_, (ctypes.c_void_p, ctypes.c_char_p)):
            return [int(bool(x)) for x in v]
        return [_value(x) for x in v]
    if isinstance(v, (ctypes.c_void_p, ctypes.c_char_p)):
        return int(bool(v.value))
    if isinstance(v, ctypes._SimpleCData):
        return _value(v.value)
    if isinstance(v, ctypes._Pointer):
        return _value(v.contents) if v else 0
    if isinstance(v, float):
        return float(v)
    if isinstance(v, (bool, int)):
        return int(v)
    if hasattr(v, "_obj"):  # ctypes.byref(...)
        return _value(v._obj)
    raise TypeError("launch record: argument of type %s" % type(v).__name__)


class Recorder:
    """Stands in ``_lib._lib``: ``calls`` is the record so far."""

    def __init__(self, real):
        self._real, self._with_stream = real, _entries_with_stream()
        self.calls, self._streams, self._wrapped = [], {}, {}

    def _describe(self, name, fn, args):
        types = fn.argtypes
        if types is None or len(types) != len(args):
            raise TypeError("launch record: %s called with %d arguments" % (name, len(args)))
        out = [name]
        for i, (tp, a) in enumerate(zip(types, args)):
            if i == len(args) - 1 and name in self._with_stream:
                out.append(["stream", self._streams.setdefault(int(a or 0), len(self._streams))])
            elif tp in _INT_TYPES:
                out.append(int(a))
            elif tp in _FLOAT_TYPES:
                out.append(float(a))
            elif tp in (ctypes.c_void_p, ctypes.c_char_p):
                out.append(int(bool(a)))  # an address (or None / 0): null or not
            else:  # POINTER(struct) / POINTER(scalar): a struct, an array of either, byref, or None
                out.append(_value(a))
        return out

    def __getattr__(self, name):
        fn = getattr(self._real, name)
        if name in SKIP:
            return fn
        w = self._wrapped.get(name)
        if w is None:
            def w(*args, _fn=fn, _name=name):
                self.calls.append(self._describe(_name, _fn, args))
                return _fn(*args)
            self._wrapped[name] = w
        return w


@contextlib.contextmanager
def recording():
    real = _lib.lib()
    rec = Recorder(real)
    _lib._lib = rec
    try:
        yield rec
    finally:
        _lib._lib = real


# ---- the cases -------------------------------------------------------------------------------------------------------------

B, BLOCKS = 2, 2


def _grid(deg=30.0):
    return regular_lat_lons(deg)


def _forecaster(deg=30.0, dtype=None, **kw):
    lat_lons = _grid(deg)
    model = gw.GraphWeatherForecaster(lat_lons, num_blocks=BLOCKS, **kw)
    deterministic_fill_(model, seed=1)
    model = model.to(DEV)
    model.auto_graph = False
    if dtype is not None:
        model.set_compute_dtype(dtype)
    return model, seeded_features(B, len(lat_lons), 102, seed=3).to(DEV)


def _twice_inference(model, *inputs, **kw):
    model.eval()
    with torch.no_grad():
        for _ in range(2):  # cold (packing, tables), then warm
            model(*inputs, **kw)
    torch.cuda.synchronize()


def _twice_training(model, *inputs, **kw):
    model.train()
    for _ in range(2):
        y = model(*inputs, **kw)
        y.backward(torch.ones_like(y))
        model.zero_grad(set_to_none=True)
    torch.cuda.synchronize()


def _inference(deg=30.0, dtype=None, det=False, streams=0, switch=None, **kw):
    def run():
        model, feats = _forecaster(deg, dtype, **kw)
        if det:
            set_deterministic(model)
        model.processor.graph_processor.streams = streams
        if switch is not None:
            setattr(ops, switch, False)
        try:
            _twice_inference(model, feats)
        finally:
            if switch is not None:
                setattr(ops, switch, True)
    return run


def _training(dtype=None, segments=0, **kw):
    def run():
        model, feats = _forecaster(30.0, dtype, **kw)
        if segments:
            model.processor.set_checkpoint_segments(segments)
        _twice_training(model, feats)
    return run


def _compositional(efficient_batching, dtype=None, train=False):
    def run():
        lat_lons = _grid()
        enc = gw.Encoder(lat_lons, efficient_batching=efficient_batching)
        proc = gw.Processor(num_blocks=BLOCKS)
        dec = gw.Decoder(lat_lons, efficient_batching=efficient_batching)
        feats = seeded_features(B, len(lat_lons), 78, seed=3).to(DEV)
        for i, m in enumerate((enc, proc, dec)):
            deterministic_fill_(m, seed=2 + i)
            m.to(DEV)
            m.train(train)
            if dtype is not None:
                set_compute_dtype(m, dtype)
        with torch.set_grad_enabled(train):
            for _ in range(2):
                x, edge_index, edge_attr = enc(feats)
                x = proc(x, edge_index, edge_attr, batch_size=B, efficient_batching=efficient_batching)
                y = dec(x, feats)
                if train:
                    y.backward(torch.ones_like(y))
        torch.cuda.synchronize()
    return run


def _graphcast(train=False, balanced=False):
    def run():
        lat_lons = _grid()
        model = gw.GraphCast(lat_lons, num_processor_blocks=BLOCKS)
        deterministic_fill_(model, seed=5)
        model = model.to(DEV)
        model.auto_graph = False
        if balanced:
            gw.GraphCastConfig.balanced_checkpointing(model)
        feats = seeded_features(B, len(lat_lons), 78, seed=4).to(DEV)
        (_twice_training if train else _twice_inference)(model, feats)
    return run


def _assimilator(train=False):
    def run():
        rs = np.random.RandomState(11)
        n_obs = 150
        llh = np.stack([rs.uniform(-90, 90, n_obs), rs.uniform(-180, 180, n_obs), rs.uniform(0, 1, n_obs)], axis=1).astype(np.float32)
        model = gw.GraphWeatherAssimilator(output_lat_lons=_grid(), analysis_dim=24, num_blocks=BLOCKS)
        deterministic_fill_(model, seed=6)
        model = model.to(DEV)
        feats = seeded_features(B, n_obs, 2, seed=7).to(DEV)
        (_twice_training if train else _twice_inference)(model, feats, torch.from_numpy(llh)[None].to(DEV))
    return run


def _regional(train=False):
    def run():
        rs = np.random.RandomState(12)
        lat_lons = [(float(a), float(b)) for a, b in zip(rs.uniform(45, 60, 90), rs.uniform(-10, 10, 90))]
        model = gw.RegionalForecasterConfig(num_blocks=BLOCKS, enable_nudging=True).build()
        deterministic_fill_(model, seed=3)
        model = model.to(DEV)
        feats = seeded_features(B, len(lat_lons), 102, seed=8).to(DEV)
        ctx = seeded_features(B, len(lat_lons), 78, seed=9).to(DEV)
        (_twice_training if train else _twice_inference)(model, feats, lat_lons, global_context=ctx)
    return run


NARROW = dict(node_dim=128, edge_dim=128, hidden_dim_processor_node=128, hidden_dim_processor_edge=128)

CASES = {
    "fp32": _inference(),
    "fp32_one_stream": _inference(streams=1),
    "fp32_deterministic": _inference(det=True),
    "fp32_encoder_two_launches": _inference(switch="ENCODER_FUSED"),
    "fp32_decoder_with_residual": _inference(switch="EDGE_STREAM"),
    "bf16": _inference(dtype=torch.bfloat16),
    "bf16_deterministic": _inference(dtype=torch.bfloat16, det=True),
    "bf16_5deg": _inference(deg=5.0, dtype=torch.bfloat16),  # a polar mesh cell with more than 64 grid nodes: split segment tiles
    "bf16x3": _inference(dtype="bf16x3"),
    "bf16x3_one_stream": _inference(dtype="bf16x3", streams=1),
    "narrow128": _inference(**NARROW),
    "thermalizer": _inference(use_thermalizer=True),
    "train_fp32": _training(),
    "train_bf16x3": _training(dtype="bf16x3"),
    "train_fp32_checkpointing": _training(use_checkpointing=True),
    "train_bf16x3_checkpointing": _training(dtype="bf16x3", use_checkpointing=True),
    "train_fp32_one_segment": _training(segments=-1),
    "train_fp32_segments_of_2": _training(segments=2),
    "train_narrow128": _training(**NARROW),
    "compositional": _compositional(False),
    "compositional_efficient_batching": _compositional(True),
    "compositional_bf16": _compositional(False, dtype=torch.bfloat16),
    "compositional_efficient_batching_bf16": _compositional(True, dtype=torch.bfloat16),
    "compositional_train": _compositional(False, train=True),
    "graphcast": _graphcast(),
    "graphcast_train_balanced_checkpointing": _graphcast(train=True, balanced=True),
    "assimilator": _assimilator(),
    "assimilator_train": _assimilator(train=True),
    "regional_nudging": _regional(),
    "regional_nudging_train": _regional(train=True),
}


def record_case(name):
    with recording() as rec:
        CASES[name]()
    return rec.calls


# ---- the golden file --------------------------------------------------------------------------------------------------------


def pack(records):
    """{case: [call, ...]} -> {"calls": [distinct calls], "cases": {case: [index, ...]}}."""
    table, index, cases = [], {}, {}
    for name, calls in records.items():
        ids = []
        for c in calls:
            key = json.dumps(c)
            if key not in index:
                index[key] = len(table)
                table.append(c)
            ids.append(index[key])
        cases[name] = ids
    return {"calls": table, "cases": cases}


def unpack(packed):
    return {name: [packed["calls"][i] for i in ids] for name, ids in packed["cases"].items()}


def load_golden(path=GOLDEN):
    with open(path) as f:
        return unpack(json.load(f))


# ---- what the records must contain to prove anything -------------------------------------------------------------------------

_EDGE = dict(e_out_layout=11, flags=17)  # positions in a gw_edge_update_forward record (entry name at 0)
_NODE_N_POST = 10  # ... of n_post in a gw_node_update_forward record


def coverage(records):
    """{route: seen?} over all records - the routes whose call sites the refactor rewrites."""
    calls = [c for cs in records.values() for c in cs]
    edge_flags = {c[_EDGE["flags"]] for c in calls if c[0] == "gw_edge_update_forward"}
    names = {c[0] for c in calls}
    E = _lib
    return {
        "edge update, flags 0": 0 in edge_flags,
        "edge update, deterministic": any(f & E.EDGE_DETERMINISTIC for f in edge_flags),
        "edge update, segment tiles": E.EDGE_SEGMENT_TILES in edge_flags,
        "edge update, segment tiles + bf16 aggregate": (E.EDGE_SEGMENT_TILES | E.EDGE_AGG_BF16K) in edge_flags,
        "edge update, split segment tiles": any(f & E.EDGE_SEGMENT_SPLIT for f in edge_flags),
        "edge update, e' as tiles": any(c[0] == "gw_edge_update_forward" and c[_EDGE["e_out_layout"]] == E.LAYOUT_EDGE_TILES_BF16
                                        for c in calls),
        "gw_encoder_fused_forward": "gw_encoder_fused_forward" in names,
        "gw_node_update_head_forward": "gw_node_update_head_forward" in names,
        "gw_mlp_post_forward": "gw_mlp_post_forward" in names,
        "node update with post products": any(c[0] == "gw_node_update_forward" and c[_NODE_N_POST] > 0 for c in calls),
        "a second stream": any(isinstance(a, list) and a[:1] == ["stream"] and a[1] >= 1 for c in calls for a in c[1:]),
    }


def main(out_path):
    records = {}
    for name in CASES:
        records[name] = record_case(name)
        print("  %-45s %5d calls" % (name, len(records[name])), flush=True)
    packed = pack(records)
    with open(out_path, "w") as f:
        json.dump(packed, f, separators=(",", ":"))
    missing = [k for k, seen in coverage(records).items() if not seen]
    print("launch records: %d cases, %d calls, %d distinct, %d bytes; routes missing: %s"
          % (len(records), sum(len(c) for c in records.values()), len(packed["calls"]), os.path.getsize(out_path), missing or "none"))
    return 1 if missing else 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1]))
