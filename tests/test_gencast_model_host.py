"""The GenCast model without a GPU: the graph builder against the arrays the reference's own files produced (tests/golden,
scripts/gen_gencast_model_golden.py), the closest-face rule against brute force, ``batch`` / ``hetero_batch``, the Preconditioner
against float64, signatures, ``state_dict`` keys and order, buffers, error messages, the alias import paths, the float32
restatement of the forward against the reference's recorded outputs, and the host-side decisions of the batch-shared launches."""
import ctypes
import inspect
import json
import os

import numpy as np
import pytest
import torch

from . import gencast_model_oracle as mo
from .cafa_oracle import fill_, params
from .test_alias import alias_modules

CASE_NAMES = tuple(mo.CASES)


@pytest.fixture(scope="module")
def tables(golden_dir):
    with open(os.path.join(golden_dir, "gencast_model_state_dict.json")) as f:
        return json.load(f)


@pytest.fixture(scope="module")
def models():
    """name -> our Denoiser on the CPU with the case's seeded weights (built once)."""
    from graph_weather_amd.gencast_model import Denoiser

    return {name: fill_(Denoiser(**mo.case_kwargs(name)), mo.CASES[name][3]) for name in CASE_NAMES}


def _golden(golden_dir, name):
    return np.load(os.path.join(golden_dir, name + ".npz"))


# ---- graphs ------------------------------------------------------------------------------------------------------------------
def test_builder_equals_the_references_graphs_case_a(golden_dir, models):
    g = _golden(golden_dir, "gencast_model_a")
    ours = mo.graph_tables(models["gencast_model_a"])
    assert set(ours) == set(mo.GRAPH_KEYS)
    assert [int(d) for d in g["dims"]] == [3, 3, 4, 4, 4]
    b = models["gencast_model_a"].graphs
    assert [b.grid_nodes_dim, b.mesh_nodes_dim, b.mesh_edges_dim, b.g2m_edges_dim, b.m2g_edges_dim] == [3, 3, 4, 4, 4]
    assert b.num_hops == 2 and ours["mesh_nodes"].shape[0] == 42 and ours["mesh_edge_index"].shape[1] == 240
    assert ours["khop_mesh_edge_index"].shape[1] == 660
    for k in mo.GRAPH_KEYS:
        want, got = g[k], ours[k].numpy()
        assert got.shape == want.shape and got.dtype == want.dtype, k
        if want.dtype == np.int64:
            assert np.array_equal(got, want), k  # integer tables exactly, edge order included
        else:
            err = np.abs(got.astype(np.float64) - want.astype(np.float64)).max()
            print("%s: max difference %.3e" % (k, err))
            assert err <= 1e-6, (k, err)


def test_builder_equals_the_references_graphs_case_b(golden_dir, models):
    g = _golden(golden_dir, "gencast_model_b")
    ours = mo.graph_tables(models["gencast_model_b"])
    assert "khop_mesh_edge_attr" not in ours  # use_edges_features=False: no k-hop edge features are computed
    assert ours["mesh_nodes"].shape[0] == 162 and ours["khop_mesh_edge_index"].shape[1] == 5460
    ends = {"g2m": ("g2m_grid_nodes", "g2m_mesh_nodes"), "m2g": ("m2g_mesh_nodes", "m2g_grid_nodes")}
    for k, v in ours.items():
        if v.dtype == torch.int64:
            s, d = ends.get(k[:3], ("mesh_nodes", "mesh_nodes"))
            assert int(g[k + "_count"]) == v.shape[1], k
            assert np.array_equal(np.bincount(v[1].numpy(), minlength=ours[d].shape[0]), g[k + "_indeg"]), k
            assert np.array_equal(np.bincount(v[0].numpy(), minlength=ours[s].shape[0]), g[k + "_outdeg"]), k
        else:
            assert list(v.shape) == list(g[k + "_shape"]), k
            err = np.abs(v.double().sum(0).numpy() - g[k + "_colsum"]).max()
            print("%s: column sums differ by %.3e over %d rows" % (k, err, v.shape[0]))
            assert err <= 1e-6 * v.shape[0], (k, err)
    assert (g["g2m_edge_index_indeg"] == 0).any()  # some mesh nodes receive nothing from the grid


def test_khop_graph_is_the_coalesced_closure():
    from graph_weather_amd import gencast_graphs as gg

    mesh = gg.get_hierarchy_of_triangular_meshes_for_sphere(1)[-1]
    s, r = gg.faces_to_edges(mesh.faces)
    n = mesh.vertices.shape[0]
    one = gg.khop_edge_index(s, r, n, 1)
    assert np.array_equal(one, np.stack([s, r])[:, np.lexsort((r, s))])
    a = np.zeros((n, n), dtype=bool)
    a[s, r] = True
    reach = a.copy()
    for hops in (2, 3):
        reach = reach | ((reach.astype(int) @ a.astype(int)) > 0)
        np.fill_diagonal(reach, False)
        got = gg.khop_edge_index(s, r, n, hops)
        assert np.array_equal(got, np.stack(np.nonzero(reach)))  # row-major, no self-loops, no duplicates


def _pole_grid():
    return np.array([0.0, 36.0, 90.0, 180.0, 270.0]), np.array([-90.0, -31.7, 0.0, 26.565, 58.28, 90.0])


def test_closest_face_rule_equals_brute_force_with_poles_and_ties():
    from graph_weather_amd import gencast_graphs as gg

    lon, lat = _pole_grid()
    for splits in (0, 1, 2):
        mesh = gg.get_hierarchy_of_triangular_meshes_for_sphere(splits)[-1]
        pos = gg._grid_positions(lat.astype(np.float32), lon.astype(np.float32))
        # points that tie by construction: the midpoints of mesh edges and the mesh vertices, pushed to the sphere
        s, r = gg.faces_to_edges(mesh.faces)
        mid = mesh.vertices[s[:40]].astype(np.float64) + mesh.vertices[r[:40]]
        pos = np.concatenate([pos, mid / np.linalg.norm(mid, axis=1, keepdims=True), mesh.vertices[:12].astype(np.float64)])
        d = mo.triangle_distances(pos, mesh.vertices, mesh.faces)
        tied = (d <= d.min(1)[:, None] + mo.TIE_TOL).sum(1)
        assert (tied >= 2).sum() >= 40 and (tied >= 5).any()  # edge midpoints tie two faces, vertices five or six
        want, least, _ = mo.closest_faces_brute(pos, mesh.vertices, mesh.faces)
        got = gg.closest_faces(pos, mesh)
        assert np.array_equal(got, want), splits
        # the property: every chosen face is within 1e-9 of the least distance, and no lower face index is
        chosen = d[np.arange(pos.shape[0]), got]
        assert (chosen <= least + mo.TIE_TOL).all()
        for i, f in enumerate(got):
            assert not (d[i, :f] <= least[i] + mo.TIE_TOL).any()


def test_point_triangle_distance_equals_the_oracles_formulation():
    from graph_weather_amd import gencast_graphs as gg

    rs = np.random.RandomState(3)
    tri = rs.standard_normal((1, 3, 3))
    pts = np.concatenate([rs.standard_normal((300, 3)) * 2, tri[0], tri[0].mean(0, keepdims=True), (tri[0][:1] + tri[0][1:2]) / 2])
    want = mo.triangle_distances(pts, tri[0], np.array([[0, 1, 2]]))[:, 0]
    n = pts.shape[0]
    got = gg.point_triangle_distance(pts, np.repeat(tri[:, 0], n, 0), np.repeat(tri[:, 1], n, 0), np.repeat(tri[:, 2], n, 0))
    assert np.abs(got - want).max() <= 1e-12


def test_m2g_edges_are_the_chosen_faces_vertices(models):
    m = models["gencast_model_a"]
    mesh = m.graphs._mesh
    from graph_weather_amd import gencast_graphs as gg

    pos = gg._grid_positions(m.graphs._grid_lat, m.graphs._grid_lon)
    want, _, _ = mo.closest_faces_brute(pos, mesh.vertices, mesh.faces)
    ei = m.m2g_edge_index.numpy()
    assert np.array_equal(ei[1], np.repeat(np.arange(pos.shape[0]), 3))
    assert np.array_equal(ei[0].reshape(-1, 3), mesh.faces[want])
    d = mo.triangle_distances(pos, mesh.vertices, mesh.faces)
    assert ((d <= d.min(1)[:, None] + mo.TIE_TOL).sum(1) >= 2).sum() == 6  # 6 of the 84 points project onto a mesh edge


def test_graph_containers_answer_the_references_accesses():
    from graph_weather_amd.gencast_graphs import GraphBuilder

    lon, lat = mo.GRIDS["gencast_model_a"]()
    g = GraphBuilder(lon, lat, splits=1)
    assert g.num_hops == 0 and not hasattr(g, "khop_mesh_graph")
    assert g.g2m_graph["grid_nodes"].x.shape == (84, 3) and g.g2m_graph["mesh_nodes"].x.shape == (42, 3)
    e = g.g2m_graph["grid_nodes", "to", "mesh_nodes"]
    assert e.edge_index.dtype == torch.int64 and e.edge_attr.shape == (e.edge_index.shape[1], 4)
    assert g.mesh_graph.x.shape == (42, 3) and g.mesh_graph.edge_attr.shape == (240, 4)
    assert g.m2g_graph["mesh_nodes", "to", "grid_nodes"].edge_index.shape == (2, 252)
    k = GraphBuilder(lon, lat, splits=1, num_hops=2, add_edge_features_to_khop=False).khop_mesh_graph
    assert k.edge_attr is None and k.edge_index.shape == (2, 660)
    assert [p for p in inspect.signature(GraphBuilder.__init__).parameters][1:] == ["grid_lon", "grid_lat", "splits", "num_hops", "device",
                                                                                  "khop_device", "add_edge_features_to_khop"]


# ---- batching and preconditioning --------------------------------------------------------------------------------------------
def test_batch_and_hetero_batch():
    from graph_weather_amd.gencast_model import batch, hetero_batch

    rs = np.random.RandomState(0)
    s, r = torch.from_numpy(rs.rand(5, 2)), torch.from_numpy(rs.rand(3, 4))
    ei = torch.tensor([[0, 4, 2, 2], [1, 2, 0, 0]])
    ea = torch.from_numpy(rs.rand(4, 3))
    for B in (1, 3):
        bs, bi, ba = batch(s, ei, ea, B)
        assert torch.equal(bs, s.repeat(B, 1)) and torch.equal(ba, ea.repeat(B, 1))
        assert torch.equal(bi, torch.cat([ei + i * 5 for i in range(B)], dim=1))
        assert batch(s, ei, None, B)[2] is None
        hs, hr, hi, ha = hetero_batch(s, r, ei, ea, B)
        assert torch.equal(hs, s.repeat(B, 1)) and torch.equal(hr, r.repeat(B, 1)) and torch.equal(ha, ea.repeat(B, 1))
        assert torch.equal(hi, torch.cat([ei + torch.tensor([[i * 5], [i * 3]]) for i in range(B)], dim=1))
        assert hetero_batch(s, r, ei, None, B)[3] is None
    assert batch(s, ei)[1] is ei and hetero_batch(s, r, ei)[2] is ei


def test_preconditioner_against_float64():
    from graph_weather_amd.gencast_model import Preconditioner, generate_isotropic_noise, sample_noise_level

    sigma = torch.tensor([[0.02], [0.5], [1.0], [3.0], [88.0]])
    for sd in (1, 0.5):
        p = Preconditioner(sigma_data=sd)
        s64 = sigma.double()
        want = (sd ** 2 / (s64 ** 2 + sd ** 2), s64 * sd / (s64 ** 2 + sd ** 2).sqrt(), 1 / (s64 ** 2 + sd ** 2).sqrt(), s64.log() / 4)
        for got, w in zip((p.c_skip(sigma), p.c_out(sigma), p.c_in(sigma), p.c_noise(sigma)), want):
            assert got.dtype == torch.float32 and (got.double() - w).abs().max() <= 4e-7 * w.abs().max()
        for got, w in zip(mo.preconditioner(sigma, sd), want):
            assert (got.double() - w).abs().max() <= 4e-7 * w.abs().max()
    assert Preconditioner().sigma_data == 1 and len(Preconditioner().state_dict()) == 0
    np.random.seed(4)
    levels = [sample_noise_level() for _ in range(200)]
    assert 0.02 <= min(levels) and max(levels) <= 88 and sample_noise_level(1.0, 1.0) == pytest.approx(1.0)
    with pytest.raises(NotImplementedError, match="torch_harmonics"):
        generate_isotropic_noise(8, 4)


# ---- the model's surface -----------------------------------------------------------------------------------------------------
def _sig(cls):
    out = []
    for name, prm in list(inspect.signature(cls.__init__).parameters.items())[1:]:
        d = prm.default
        out.append([name, "<required>" if d is inspect.Parameter.empty else
                    (d if isinstance(d, (bool, int, float, list, type(None))) else str(d))])
    return out


def test_signatures_equal_the_references(tables):
    from graph_weather_amd.gencast_graphs import GraphBuilder
    from graph_weather_amd.gencast_model import Denoiser, DenoiserConfig, Preconditioner

    for cls in (Denoiser, GraphBuilder, Preconditioner, DenoiserConfig):
        assert _sig(cls) == tables["signature"][cls.__name__], cls.__name__


@pytest.mark.parametrize("name", CASE_NAMES)
def test_state_dict_keys_order_and_buffers(tables, models, name):
    m = models[name]
    assert {k: list(v.shape) for k, v in m.state_dict().items()} == tables["state_dict"][name]
    assert list(m.state_dict()) == list(tables["state_dict"][name])  # the order too
    if name == "gencast_model_a":
        assert len(m.state_dict()) == 98
    assert list(m._buffers) == tables["buffers"]  # registration order (the two mesh node tables are one tensor)
    assert (m.khop_mesh_edge_attr is None) == (not m.use_edges_features)
    assert set(m._non_persistent_buffers_set) == set(tables["buffers"])
    assert m.num_lon == len(mo.GRIDS[name]()[0]) and m.num_lat == len(mo.GRIDS[name]()[1])
    assert m.precs.sigma_data == 1.0 and m.use_edges_features == mo.CASES[name][0].get("use_edges_features", True)


def test_config_builds_the_model_and_hub_mixin():
    from graph_weather_amd.gencast_model import Denoiser, DenoiserConfig

    lon, lat = mo.GRIDS["gencast_model_a"]()
    cfg = DenoiserConfig(grid_lon=lon, grid_lat=lat, input_features_dim=3, output_features_dim=2, splits=1, num_hops=1, num_blocks=1,
                         hidden_dims=[8, 8])
    assert DenoiserConfig(lon, lat, 1, 1).hidden_dims == [512, 512]
    m = cfg.build()
    assert isinstance(m, Denoiser) and len(m.processor.cond_transformers) == 1
    try:
        from huggingface_hub import PyTorchModelHubMixin
    except Exception:
        return
    assert isinstance(m, PyTorchModelHubMixin)


def test_error_messages(models):
    from graph_weather_amd.gencast_model import Denoiser

    lon, lat = mo.GRIDS["gencast_model_a"]()
    kw = dict(grid_lon=lon, grid_lat=lat, input_features_dim=3, output_features_dim=2, hidden_dims=[8, 8], num_blocks=1, splits=1,
              num_hops=1)
    with pytest.raises(ValueError, match="Sparse processor don't support edges features."):
        Denoiser(sparse=True, **kw)
    with pytest.raises(ValueError, match="Please install DGL to use sparsity."):
        Denoiser(sparse=True, use_edges_features=False, **kw)
    m = models["gencast_model_a"]
    z, x, s = mo.case_inputs("gencast_model_a")
    msg = ("The shapes of the input tensors don't match with the initialization parameters: expected (2, 12, 7, 6) for prev_inputs, "
           "(2, 12, 7, 2) for targets and (2, 1) for noise_levels.")
    for bad in ((z[:, :, :, :1], x, s), (z, x.transpose(1, 2), s), (z, x, s[:, 0])):
        with pytest.raises(ValueError) as err:
            m(*bad)
        assert str(err.value) == msg
    with pytest.raises(ValueError, match="All the noise levels must be strictly positive."):
        m(z, x, -s)
    with pytest.raises(RuntimeError, match="HIP device"):  # the reference's .any(): one positive level passes the check
        m(z, x, s * torch.tensor([[1.0], [-1.0]]))


def test_alias_imports_give_the_model_classes():
    from graph_weather_amd import gencast_graphs, gencast_model

    with alias_modules():
        from graph_weather.models.gencast import Denoiser, GraphBuilder, generate_isotropic_noise
        from graph_weather.models.gencast.denoiser import Denoiser as D2, DenoiserConfig
        from graph_weather.models.gencast.graph import grid_mesh_connectivity, icosahedral_mesh, model_utils
        from graph_weather.models.gencast.graph.graph_builder import GraphBuilder as G2
        from graph_weather.models.gencast.utils.batching import batch, hetero_batch
        from graph_weather.models.gencast.utils.noise import Preconditioner, sample_noise_level
    assert Denoiser is D2 is gencast_model.Denoiser and DenoiserConfig is gencast_model.DenoiserConfig
    assert GraphBuilder is G2 is gencast_graphs.GraphBuilder
    assert (batch, hetero_batch, Preconditioner, sample_noise_level, generate_isotropic_noise) == (
        gencast_model.batch, gencast_model.hetero_batch, gencast_model.Preconditioner, gencast_model.sample_noise_level,
        gencast_model.generate_isotropic_noise)
    assert icosahedral_mesh.faces_to_edges is gencast_graphs.faces_to_edges
    assert grid_mesh_connectivity.radius_query_indices is gencast_graphs.radius_query_indices
    assert model_utils.get_graph_spatial_features is gencast_graphs.get_graph_spatial_features


# ---- the restatement against the reference's outputs -------------------------------------------------------------------------
@pytest.mark.parametrize("name", CASE_NAMES)
def test_float32_restatement_gives_the_references_output(golden_dir, models, name):
    """The oracle the GPU tests use, on our graphs and the seeded weights, against what the reference's own Denoiser computed."""
    want = torch.from_numpy(_golden(golden_dir, name)["out"])
    m = models[name]
    got = mo.denoiser_forward(params(m, torch.float32), mo.CASES[name][0], mo.graph_tables(m), *mo.case_inputs(name))
    err = (got - want).abs().max().item()
    print("%s: float32 restatement against the reference's output: %.3e (maximum %.3e)" % (name, err, want.abs().max().item()))
    assert got.shape == want.shape and err <= 2e-5 * max(want.abs().max().item(), 1.0)


# ---- host-side decisions of the batch-shared launches ------------------------------------------------------------------------
def test_edge_table_stride_routing():
    from graph_weather_amd.gencast import edge_table_stride

    assert edge_table_stride(None, 660, 4) == 0  # no table
    assert edge_table_stride(660, 660, 4) == 0  # one table shared by the copies
    assert edge_table_stride(2640, 660, 4) == 660  # one per copy
    assert edge_table_stride(660, 660, 1) == 0
    assert edge_table_stride(0, 0, 3) == 0
    with pytest.raises(RuntimeError, match="660 rows .shared. or 2640"):
        edge_table_stride(1320, 660, 4)


def test_new_entry_points_refuse_bad_arguments_on_the_host():
    from graph_weather_amd import _lib

    L = _lib.lib()
    buf = (ctypes.c_float * 4096)()
    p = ctypes.addressof(buf)
    att = [4, 4, 8, 2, 4, p, p, p, p, 8, p, 8, p, 8, p, 8, 0, p, 8, None, 8, p, None]
    assert L.gw_graph_attention_batched_forward(0, 0, *att) != 0  # batch 0
    assert L.gw_graph_attention_batched_forward(2, 5, *att) != 0  # a stride between 0 and E: the tables would overlap
    assert b"gw_graph_attention_batched_forward" in L.gw_last_error()
    assert L.gw_graph_attention_batched_forward(2, 0, 4, 4, 0, *att[3:]) == 0  # no edges: nothing is launched
    assert L.gw_cond_layernorm_grouped_forward(8, 4, 0, 0, p, 4, p, 4, p, 4, p, 4, None) != 0  # rows_per_group 0
    assert L.gw_cond_layernorm_grouped_forward(0, 4, 0, 3, p, 4, p, 4, p, 4, p, 4, None) == 0  # no rows
    assert L.gw_cond_layernorm_grouped_workspace_bytes(600, 12, 300) == (600 * 2 + 2 * 2 * 2 * 12) * 4
    assert L.gw_cond_layernorm_grouped_workspace_bytes(600, 12, 0) == 0
    assert L.gw_cond_layernorm_grouped_backward(8, 4, 0, 4, p, 4, p, 4, p, 4, p, 4, p, 16, p, 4, p, p, 4, None) != 0  # workspace too small
    assert b"workspace" in L.gw_last_error()
    assert L.gw_gencast_precond_input_forward(0, 11, 2, 6, 3, 1.0, p, p, 2, p, 6, p, 3, p, 11, p, None) != 0  # batch 0
    assert L.gw_gencast_precond_input_forward(3, 11, 2, 6, 3, 1.0, p, p, 2, p, 6, p, 3, p, 10, p, None) != 0  # ld_out too small
    assert L.gw_gencast_precond_input_backward(3, 11, 2, 6, 1.0, p, p, 8, None, 2, None, 6, None) != 0  # nothing wanted
    assert L.gw_gencast_precond_output_forward(3, 11, 2, 0.0, p, p, 2, p, 2, p, 2, None) != 0  # sigma_data 0
    assert L.gw_gencast_precond_output_backward(3, 11, 2, 1.0, p, p, 1, p, 2, p, 2, None) != 0  # ld_dout too small
