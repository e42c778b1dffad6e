"""Write tests/golden/fengwu_*.npz and fengwu_state_dict.json from the reference's own ImageMetaModel, WrapperImageModel,
MetaModel and WrapperMetaModel.

Run from the repository root, on the CPU, with the reference tree and einops present: ``python scripts/gen_fengwu_golden.py``.
The reference file is loaded read-only by path under oracle.refload.REF_ROOT.  Its two torch_geometric imports get stand-ins
of their documented behaviour: ``nn.pool.knn(x, y, k)`` -> the assignment [2, n_y * k] (row 0 target, row 1 source) under the
tie rule of tests/fengwu_oracle.knn_assign (the real kd-tree leaves ties open), ``utils.scatter(src, index, dim, dim_size,
reduce="sum")`` -> zeros.index_add_.  Weights come from tests/fengwu_oracle.fill_ (per-key seeded) and inputs from
numpy.RandomState(seed): the fixtures hold the seed, meta and the output - no weights, no inputs.
"""
import importlib.util
import json
import os
import sys
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT]

from tests import fengwu_oracle as fo  # noqa: E402
from oracle.refload import REF_ROOT  # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden")


def _load_reference():
    def knn(x, y, k, num_workers=1):
        assert k == fo.K
        a = fo.knn_assign(x, y)
        return torch.stack([torch.arange(y.shape[0]).repeat_interleave(k), a.reshape(-1)])

    def scatter(src, index, dim=0, dim_size=None, reduce="sum"):
        assert dim == 0 and reduce == "sum"
        out = torch.zeros((dim_size,) + tuple(src.shape[1:]), dtype=src.dtype)
        return out.index_add_(0, index, src)

    names = ("torch_geometric", "torch_geometric.nn", "torch_geometric.nn.pool", "torch_geometric.utils")
    saved = {n: sys.modules.get(n) for n in names}
    mods = {n: types.ModuleType(n) for n in names}
    mods["torch_geometric.nn.pool"].knn = knn
    mods["torch_geometric.utils"].scatter = scatter
    sys.modules.update(mods)
    try:
        path = os.path.join(REF_ROOT, "graph_weather", "models", "fengwu_ghr", "layers.py")
        spec = importlib.util.spec_from_file_location("_reference_fengwu_layers", path)
        mod = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(mod)
    finally:
        for n, m in saved.items():
            if m is None:
                sys.modules.pop(n, None)
            else:
                sys.modules[n] = m
    return mod


def _save(name, seed, meta, out):
    np.savez_compressed(os.path.join(GOLDEN, name + ".npz"), seed=np.int64(seed), meta=np.array(meta, dtype=np.int64),
                        out=out.numpy().astype(np.float32))


def _flat(cfg):
    vals = []
    for k in ("image_size", "patch_size"):
        vals += list(fo.pair(cfg[k]))
    return vals + [cfg[k] for k in ("depth", "heads", "mlp_dim", "channels", "dim_head")]


def main():
    ref = _load_reference()
    lat_lons = fo.lat_lons_5deg()
    tables = {}
    for name, (cfg, batch, seed) in fo.IMAGE_CASES.items():
        model = fo.fill_(ref.ImageMetaModel(**cfg), seed)
        with torch.no_grad():
            out = model(fo.image_input(cfg, batch, seed))
        _save(name, seed, _flat(cfg) + [batch], out)
        tables["ImageMetaModel:" + name] = model
    for name, (cfg, scale, batch, seed) in fo.WRAPPER_IMAGE_CASES.items():
        model = fo.fill_(ref.WrapperImageModel(ref.ImageMetaModel(**cfg), scale), seed)
        with torch.no_grad():
            out = model(fo.image_input(cfg, batch, seed, scale))
        _save(name, seed, _flat(cfg) + list(fo.pair(scale)) + [batch], out)
        tables["WrapperImageModel:" + name] = model
    for name, (cfg, batch, seed) in fo.META_CASES.items():
        model = fo.fill_(ref.MetaModel(lat_lons, **cfg), seed)
        with torch.no_grad():
            out = model(fo.rows_input(cfg, batch, seed, len(lat_lons)))
        _save(name, seed, _flat(cfg) + [batch, len(lat_lons)], out)
        tables["MetaModel:" + name] = model
    for name, (cfg, scale, batch, seed) in fo.WRAPPER_META_CASES.items():
        model = fo.fill_(ref.WrapperMetaModel(lat_lons, ref.MetaModel(lat_lons, **cfg), scale), seed)
        with torch.no_grad():
            out = model(fo.rows_input(cfg, batch, seed, len(lat_lons)))
        _save(name, seed, _flat(cfg) + list(fo.pair(scale)) + [batch, len(lat_lons)], out)
        tables["WrapperMetaModel:" + name] = model
    out = {k: {n: list(v.shape) for n, v in m.state_dict().items()} for k, m in tables.items()}
    with open(os.path.join(GOLDEN, "fengwu_state_dict.json"), "w") as f:
        json.dump(out, f, indent=0, sort_keys=False)


if __name__ == "__main__":
    main()
