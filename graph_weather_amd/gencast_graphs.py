"""GenCast's graphs (graph_weather/models/gencast/graph of the reference) on numpy and scipy: the icosphere hierarchy, the
grid-to-mesh radius query, the mesh, the mesh-to-grid triangles, the k-hop closure and the spatial features of all four, in the
reference's vertex, face and edge order.  Host code only; ``GraphBuilder`` leaves torch tensors on ``device``.

What the reference takes from trimesh, xarray, dacite and torch_geometric.data is restated: ``Data`` / ``HeteroData`` are small
containers that answer the accesses ``Denoiser._register_graph`` makes, the k-hop closure runs on ``scipy.sparse`` (repeated
products, self-loops removed, indices in coalesced row-major order) and the spatial features are computed under the one
configuration the reference fixes (node latitude and longitude, relative positions in the receiver's local coordinates on both
axes, no node positions).

One step is a rule of this package: the triangle that "contains" a grid point.  The reference asks
``trimesh.proximity.closest_point`` for the closest face of the flat-faced mesh; a point of the unit sphere that projects onto
an edge of that mesh is exactly as far from both adjacent faces and trimesh's pick is an implementation detail.  Here the exact
point-to-triangle distance is computed in float64 and, among the faces within ``TIE_TOL`` = 1e-9 of the minimum, the lowest face
index is taken (``closest_faces``).  For such tied points the reference may pick the other face adjacent to the same mesh edge.
"""
from __future__ import annotations

from typing import List, NamedTuple, Optional, Tuple

import numpy as np
import torch

__all__ = ["TriangularMesh", "get_icosahedron", "get_hierarchy_of_triangular_meshes_for_sphere", "faces_to_edges",
           "radius_query_indices", "in_mesh_triangle_indices", "closest_faces", "point_triangle_distance", "TIE_TOL",
           "get_graph_spatial_features", "get_bipartite_graph_spatial_features", "lat_lon_deg_to_spherical", "spherical_to_lat_lon",
           "cartesian_to_spherical", "spherical_to_cartesian", "khop_edge_index", "Data", "HeteroData", "GraphBuilder"]

TIE_TOL = 1e-9
RADIUS_QUERY_FRACTION_EDGE_LENGTH = 0.6

# the regular icosahedron's faces, counter-clockwise seen from outside (the table GraphCast and the reference use)
_ICOSAHEDRON_FACES = ((0, 1, 2), (0, 6, 1), (8, 0, 2), (8, 4, 0), (3, 8, 2), (3, 2, 7), (7, 2, 1), (0, 4, 6), (4, 11, 6), (6, 11, 5),
                      (1, 5, 7), (4, 10, 11), (4, 8, 10), (10, 8, 3), (10, 3, 9), (11, 10, 9), (11, 9, 5), (5, 9, 7), (9, 3, 7),
                      (1, 6, 5))


class TriangularMesh(NamedTuple):
    vertices: np.ndarray  # [num_vertices, 3] float32, unit norm
    faces: np.ndarray     # [num_faces, 3] int32


# ---------------------------------------------------------------------------------------------------------------------
# icosahedral_mesh.py
# ---------------------------------------------------------------------------------------------------------------------
def get_icosahedron() -> TriangularMesh:
    """The regular icosahedron with circumscribed unit sphere, rotated about y so that a face (not an edge) lies on top."""
    from scipy.spatial import transform

    phi = (1 + np.sqrt(5)) / 2
    vertices = []
    for c1 in (1.0, -1.0):
        for c2 in (phi, -phi):
            vertices += [(c1, c2, 0.0), (0.0, c1, c2), (c2, 0.0, c1)]
    vertices = np.array(vertices, dtype=np.float32)
    vertices /= np.linalg.norm([1.0, phi])
    angle_between_faces = 2 * np.arcsin(phi / np.sqrt(3))
    rotation = transform.Rotation.from_euler(seq="y", angles=(np.pi - angle_between_faces) / 2)
    vertices = np.dot(vertices, rotation.as_matrix())
    return TriangularMesh(vertices=vertices.astype(np.float32), faces=np.array(_ICOSAHEDRON_FACES, dtype=np.int32))


def _split_faces(mesh: TriangularMesh) -> TriangularMesh:
    """Every face into four: the new vertices are the edge midpoints pushed back to the unit sphere, numbered in the order the
    faces first ask for them (edge (1, 2), then (2, 3), then (3, 1) of each face); children (1, 12, 31), (12, 2, 23),
    (31, 23, 3), (12, 23, 31) keep the orientation."""
    parents = mesh.vertices
    all_vertices = list(parents)
    child_of = {}

    def child(i, j):
        key = (i, j) if i < j else (j, i)
        if key not in child_of:
            pos = parents[[i, j]].mean(0)
            pos /= np.linalg.norm(pos)
            child_of[key] = len(all_vertices)
            all_vertices.append(pos)
        return child_of[key]

    faces = []
    for i1, i2, i3 in mesh.faces:
        i12, i23, i31 = child(i1, i2), child(i2, i3), child(i3, i1)
        faces += [[i1, i12, i31], [i12, i2, i23], [i31, i23, i3], [i12, i23, i31]]
    return TriangularMesh(vertices=np.array(all_vertices), faces=np.array(faces, dtype=np.int32))


def get_hierarchy_of_triangular_meshes_for_sphere(splits: int) -> List[TriangularMesh]:
    meshes = [get_icosahedron()]
    for _ in range(splits):
        meshes.append(_split_faces(meshes[-1]))
    return meshes


def faces_to_edges(faces: np.ndarray) -> Tuple[np.ndarray, np.ndarray]:
    """Face (a, b, c) gives the edges a->b, b->c, c->a: all first edges, then all second, then all third."""
    assert faces.ndim == 2 and faces.shape[-1] == 3
    return (np.concatenate([faces[:, 0], faces[:, 1], faces[:, 2]]), np.concatenate([faces[:, 1], faces[:, 2], faces[:, 0]]))


# ---------------------------------------------------------------------------------------------------------------------
# model_utils.py (the coordinate helpers and the two feature functions; the xarray helpers are not restated)
# ---------------------------------------------------------------------------------------------------------------------
def lat_lon_deg_to_spherical(node_lat, node_lon):
    return np.deg2rad(node_lon), np.deg2rad(90 - node_lat)


def spherical_to_lat_lon(phi, theta):
    return 90 - np.rad2deg(theta), np.mod(np.rad2deg(phi), 360)


def cartesian_to_spherical(x, y, z):
    phi = np.arctan2(y, x)
    with np.errstate(invalid="ignore"):
        theta = np.arccos(z)
    return phi, theta


def spherical_to_cartesian(phi, theta):
    return (np.cos(phi) * np.sin(theta), np.sin(phi) * np.sin(theta), np.cos(theta))


def _node_features(phi, theta):
    return np.stack([np.cos(theta), np.cos(phi), np.sin(phi)], axis=-1)


def _relative_positions(send_phi, send_theta, senders, recv_phi, recv_theta, receivers):
    """Sender minus receiver position in the receiver's local frame: rotated about z to longitude 0, then about y to latitude 0."""
    from scipy.spatial import transform

    send_pos = np.stack(spherical_to_cartesian(send_phi, send_theta), axis=-1)
    recv_pos = np.stack(spherical_to_cartesian(recv_phi, recv_theta), axis=-1)
    rotations = transform.Rotation.from_euler("zy", np.stack([-recv_phi, -recv_theta + np.pi / 2], axis=1)).as_matrix()
    edge_rot = rotations[receivers]
    recv_rot = np.einsum("bji,bi->bj", edge_rot, recv_pos[receivers])
    send_rot = np.einsum("bji,bi->bj", edge_rot, send_pos[senders])
    return send_rot - recv_rot


def _edge_features(relative_position, normalization: Optional[float]):
    distances = np.linalg.norm(relative_position, axis=-1, keepdims=True)
    if normalization is None:
        normalization = distances.max()
    return np.concatenate([distances / normalization, relative_position / normalization], axis=-1)


def get_graph_spatial_features(*, node_lat, node_lon, senders, receivers) -> Tuple[np.ndarray, np.ndarray]:
    """(node features [n, 3] = cos(theta), cos(phi), sin(phi); edge features [E, 4] = length and relative position, both over the
    longest edge)."""
    phi, theta = lat_lon_deg_to_spherical(node_lat, node_lon)
    senders, receivers = np.asarray(senders), np.asarray(receivers)
    rel = _relative_positions(phi, theta, senders, phi, theta, receivers)
    return _node_features(phi, theta), _edge_features(rel, None)


def get_bipartite_graph_spatial_features(*, senders_node_lat, senders_node_lon, senders, receivers_node_lat, receivers_node_lon,
                                         receivers, edge_normalization_factor: Optional[float] = None):
    """(sender node features, receiver node features, edge features) of a graph whose two ends live in different tables."""
    assert receivers_node_lat.dtype == senders_node_lat.dtype
    s_phi, s_theta = lat_lon_deg_to_spherical(senders_node_lat, senders_node_lon)
    r_phi, r_theta = lat_lon_deg_to_spherical(receivers_node_lat, receivers_node_lon)
    rel = _relative_positions(s_phi, s_theta, np.asarray(senders), r_phi, r_theta, np.asarray(receivers))
    return _node_features(s_phi, s_theta), _node_features(r_phi, r_theta), _edge_features(rel, edge_normalization_factor)


# ---------------------------------------------------------------------------------------------------------------------
# grid_mesh_connectivity.py
# ---------------------------------------------------------------------------------------------------------------------
def _grid_positions(grid_latitude: np.ndarray, grid_longitude: np.ndarray) -> np.ndarray:
    """[num_lat * num_lon, 3] unit vectors, latitude-major."""
    phi, theta = np.meshgrid(np.deg2rad(grid_longitude), np.deg2rad(90 - grid_latitude))
    return np.stack([np.cos(phi) * np.sin(theta), np.sin(phi) * np.sin(theta), np.cos(theta)], axis=-1).reshape([-1, 3])


def radius_query_indices(*, grid_latitude, grid_longitude, mesh: TriangularMesh, radius: float):
    """(grid indices, mesh indices) of the pairs no further apart than ``radius`` (straight line), grid point by grid point in the
    order ``cKDTree.query_ball_point`` lists each point's mesh vertices."""
    from scipy.spatial import cKDTree

    found = cKDTree(mesh.vertices).query_ball_point(x=_grid_positions(grid_latitude, grid_longitude), r=radius)
    grid_ix = [np.repeat(i, len(nb)) for i, nb in enumerate(found)]
    return np.concatenate(grid_ix, axis=0).astype(int), np.concatenate(list(found), axis=0).astype(int)


def point_triangle_distance(p: np.ndarray, a: np.ndarray, b: np.ndarray, c: np.ndarray) -> np.ndarray:
    """Exact distance of the points p [n, 3] from the triangles (a, b, c) [n, 3] each, float64: the closest point by Voronoi region
    (vertex, edge or interior) of the triangle."""
    p, a, b, c = (np.asarray(t, dtype=np.float64) for t in (p, a, b, c))
    ab, ac = b - a, c - a
    ap, bp, cp = p - a, p - b, p - c
    d1, d2 = (ab * ap).sum(1), (ac * ap).sum(1)
    d3, d4 = (ab * bp).sum(1), (ac * bp).sum(1)
    d5, d6 = (ab * cp).sum(1), (ac * cp).sum(1)
    vc, vb, va = d1 * d4 - d3 * d2, d5 * d2 - d1 * d6, d3 * d6 - d5 * d4

    def ratio(num, den):
        return (num / np.where(den == 0.0, 1.0, den))[:, None]

    den = va + vb + vc
    q = a + ab * ratio(vb, den) + ac * ratio(vc, den)  # interior; the regions below overwrite it, the first listed last
    for mask, point in (
            ((va <= 0) & (d4 - d3 >= 0) & (d5 - d6 >= 0), b + (c - b) * ratio(d4 - d3, (d4 - d3) + (d5 - d6))),  # edge bc
            ((vb <= 0) & (d2 >= 0) & (d6 <= 0), a + ac * ratio(d2, d2 - d6)),  # edge ac
            ((d6 >= 0) & (d5 <= d6), c),
            ((vc <= 0) & (d1 >= 0) & (d3 <= 0), a + ab * ratio(d1, d1 - d3)),  # edge ab
            ((d3 >= 0) & (d4 <= d3), b),
            ((d1 <= 0) & (d2 <= 0), a)):
        q = np.where(mask[:, None], point, q)
    return np.linalg.norm(p - q, axis=1)


def closest_faces(points: np.ndarray, mesh: TriangularMesh) -> np.ndarray:
    """The face of ``mesh`` closest to every point [n, 3]: among the faces within TIE_TOL of the least exact distance, the lowest
    face index.  Candidates are pruned with a KD-tree without changing that result: the closest face is no further than the nearest
    vertex (distance d0), so each of its vertices is within d0 + (longest edge) of the point - only faces with such a vertex are
    measured."""
    from scipy.spatial import cKDTree

    points = np.asarray(points, dtype=np.float64)
    verts, faces = mesh.vertices.astype(np.float64), mesh.faces.astype(np.int64)
    n_faces = faces.shape[0]
    s, r = faces_to_edges(faces)
    longest = np.linalg.norm(verts[s] - verts[r], axis=-1).max()
    tree = cKDTree(verts)
    d0, _ = tree.query(points)
    near = tree.query_ball_point(points, r=d0 + longest + 2 * TIE_TOL)
    # vertex -> incident faces (CSR)
    order = np.argsort(faces.reshape(-1), kind="stable")
    face_of = order // 3
    starts = np.concatenate([[0], np.cumsum(np.bincount(faces.reshape(-1), minlength=verts.shape[0]))])
    out = np.empty(points.shape[0], dtype=np.int64)
    chunk = 8192
    for p0 in range(0, points.shape[0], chunk):
        p1 = min(p0 + chunk, points.shape[0])
        pt = np.concatenate([np.full(len(nb), i, dtype=np.int64) for i, nb in zip(range(p0, p1), near[p0:p1])])
        vx = np.concatenate([np.asarray(nb, dtype=np.int64) for nb in near[p0:p1]])
        cnt = starts[vx + 1] - starts[vx]
        pair_pt = np.repeat(pt, cnt)
        offs = np.arange(cnt.sum()) - np.repeat(np.cumsum(cnt) - cnt, cnt)
        pair_face = face_of[np.repeat(starts[vx], cnt) + offs]
        key = np.unique(pair_pt * n_faces + pair_face)  # sorted by (point, face)
        kp, kf = key // n_faces, key % n_faces
        dist = point_triangle_distance(points[kp], verts[faces[kf, 0]], verts[faces[kf, 1]], verts[faces[kf, 2]])
        first = np.concatenate([[0], np.flatnonzero(np.diff(kp)) + 1])
        least = np.minimum.reduceat(dist, first)
        tied = dist <= np.repeat(least, np.diff(np.concatenate([first, [kp.size]]))) + TIE_TOL
        out[p0:p1] = np.minimum.reduceat(np.where(tied, kf, n_faces), first)
    return out


def in_mesh_triangle_indices(*, grid_latitude, grid_longitude, mesh: TriangularMesh):
    """(grid indices, mesh indices), three edges per grid point: the vertices of its closest face (``closest_faces``)."""
    positions = _grid_positions(grid_latitude, grid_longitude)
    mesh_ix = mesh.faces[closest_faces(positions, mesh)]
    grid_ix = np.tile(np.arange(positions.shape[0]).reshape([-1, 1]), [1, 3])
    return grid_ix.reshape([-1]), mesh_ix.reshape([-1])


def khop_edge_index(senders: np.ndarray, receivers: np.ndarray, num_nodes: int, num_hops: int) -> np.ndarray:
    """[2, E_k] int64: the pairs joined by a walk of at most ``num_hops`` mesh edges, without self-loops, in coalesced row-major
    order (A_1 = A; A_k = A_{k-1} + A_{k-1} A with the diagonal removed and the values reset to 1)."""
    from scipy import sparse

    ones = np.ones(len(senders), dtype=np.float32)
    adj = sparse.csr_matrix((ones, (np.asarray(senders, dtype=np.int64), np.asarray(receivers, dtype=np.int64))),
                            shape=(num_nodes, num_nodes))
    adj.sum_duplicates()
    adj_k = adj.copy()
    for _ in range(num_hops - 1):
        adj_k = (adj_k + adj_k @ adj).tocoo()
        keep = adj_k.row != adj_k.col
        adj_k = sparse.csr_matrix((np.ones(int(keep.sum()), dtype=np.float32), (adj_k.row[keep], adj_k.col[keep])),
                                  shape=(num_nodes, num_nodes))
        adj_k.sum_duplicates()
    adj_k.sort_indices()
    coo = adj_k.tocoo()
    return np.stack([coo.row, coo.col]).astype(np.int64)


# ---------------------------------------------------------------------------------------------------------------------
# the graph containers and graph_builder.py
# ---------------------------------------------------------------------------------------------------------------------
class _Store:
    """The attributes of one node or edge type."""

    x = None
    edge_index = None
    edge_attr = None

    def __repr__(self):
        return "_Store(%s)" % ", ".join("%s=%s" % (k, tuple(v.shape)) for k, v in vars(self).items() if v is not None)


class Data(_Store):
    """A homogeneous graph: ``x``, ``edge_index``, ``edge_attr`` (None when absent)."""

    def __init__(self, x=None, edge_index=None, edge_attr=None):
        self.x, self.edge_index, self.edge_attr = x, edge_index, edge_attr


class HeteroData:
    """A typed graph: ``g["grid_nodes"].x``, ``g["grid_nodes", "to", "mesh_nodes"].edge_index`` / ``.edge_attr``; a type exists
    from its first access."""

    def __init__(self):
        self._stores = {}

    def __getitem__(self, key) -> _Store:
        return self._stores.setdefault(key, _Store())

    @property
    def node_types(self):
        return [k for k in self._stores if isinstance(k, str)]

    @property
    def edge_types(self):
        return [k for k in self._stores if isinstance(k, tuple)]


def _max_edge_distance(mesh: TriangularMesh):
    senders, receivers = faces_to_edges(mesh.faces)
    return np.linalg.norm(mesh.vertices[senders] - mesh.vertices[receivers], axis=-1).max()


class GraphBuilder:
    """GenCast's graphs (graph_builder.py): ``g2m_graph`` (grid to mesh, radius query at 0.6 of the finest mesh's longest edge),
    ``mesh_graph``, ``m2g_graph`` (mesh to grid, the three vertices of each grid point's closest face: see the module docstring
    for the tie rule) and - with ``num_hops`` > 0 - ``khop_mesh_graph``; ``grid_nodes_dim``, ``mesh_nodes_dim``,
    ``mesh_edges_dim``, ``g2m_edges_dim``, ``m2g_edges_dim``.  Grid nodes are ordered latitude-major."""

    def __init__(self, grid_lon: np.ndarray, grid_lat: np.ndarray, splits: int = 5, num_hops: int = 0,
                 device: torch.device = torch.device("cpu"), khop_device: torch.device = torch.device("cpu"),
                 add_edge_features_to_khop=True):
        self.add_edge_features_to_khop = add_edge_features_to_khop
        self.device = device
        self.khop_device = khop_device  # (kept for the signature: the closure runs on scipy.sparse on the host)
        self._mesh = get_hierarchy_of_triangular_meshes_for_sphere(splits)[-1]
        self._query_radius = _max_edge_distance(self._mesh) * RADIUS_QUERY_FRACTION_EDGE_LENGTH
        self._mesh2grid_edge_normalization_factor = None
        self.grid_nodes_dim = self.mesh_nodes_dim = self.mesh_edges_dim = self.g2m_edges_dim = self.m2g_edges_dim = None

        grid_lat, grid_lon = np.asarray(grid_lat), np.asarray(grid_lon)
        self._grid_lat, self._grid_lon = grid_lat.astype(np.float32), grid_lon.astype(np.float32)
        self._num_grid_nodes = grid_lat.shape[0] * grid_lon.shape[0]
        nodes_lon, nodes_lat = np.meshgrid(grid_lon, grid_lat)
        self._grid_nodes_lon = nodes_lon.reshape([-1]).astype(np.float32)
        self._grid_nodes_lat = nodes_lat.reshape([-1]).astype(np.float32)

        self._num_mesh_nodes = self._mesh.vertices.shape[0]
        v = self._mesh.vertices
        mesh_lat, mesh_lon = spherical_to_lat_lon(*cartesian_to_spherical(v[:, 0], v[:, 1], v[:, 2]))
        self._mesh_nodes_lat, self._mesh_nodes_lon = mesh_lat.astype(np.float32), mesh_lon.astype(np.float32)

        self.g2m_graph = self._init_grid2mesh_graph()
        self.mesh_graph = self._init_mesh_graph()
        self.m2g_graph = self._init_mesh2grid_graph()
        self.num_hops = num_hops
        if num_hops > 0:
            self.khop_mesh_graph = self._init_khop_mesh_graph()

    def _f32(self, a):
        return torch.tensor(a, dtype=torch.float32, device=self.device)

    def _ix(self, senders, receivers):
        return torch.tensor(np.stack([senders, receivers]), dtype=torch.long, device=self.device)

    def _init_grid2mesh_graph(self) -> HeteroData:
        senders, receivers = radius_query_indices(grid_latitude=self._grid_lat, grid_longitude=self._grid_lon, mesh=self._mesh,
                                                  radius=self._query_radius)
        grid_x, mesh_x, edge_attr = get_bipartite_graph_spatial_features(
            senders_node_lat=self._grid_nodes_lat, senders_node_lon=self._grid_nodes_lon, receivers_node_lat=self._mesh_nodes_lat,
            receivers_node_lon=self._mesh_nodes_lon, senders=senders, receivers=receivers, edge_normalization_factor=None)
        self.grid_nodes_dim, self.mesh_nodes_dim, self.g2m_edges_dim = grid_x.shape[1], mesh_x.shape[1], edge_attr.shape[1]
        g = HeteroData()
        g["grid_nodes"].x = self._f32(grid_x)
        g["mesh_nodes"].x = self._f32(mesh_x)
        g["grid_nodes", "to", "mesh_nodes"].edge_index = self._ix(senders, receivers)
        g["grid_nodes", "to", "mesh_nodes"].edge_attr = self._f32(edge_attr)
        return g

    def _init_mesh_graph(self) -> Data:
        senders, receivers = faces_to_edges(self._mesh.faces)
        node_x, edge_attr = get_graph_spatial_features(node_lat=self._mesh_nodes_lat, node_lon=self._mesh_nodes_lon, senders=senders,
                                                       receivers=receivers)
        self.mesh_edges_dim = edge_attr.shape[1]
        return Data(x=self._f32(node_x), edge_attr=self._f32(edge_attr), edge_index=self._ix(senders, receivers))

    def _init_mesh2grid_graph(self) -> HeteroData:
        receivers, senders = in_mesh_triangle_indices(grid_latitude=self._grid_lat, grid_longitude=self._grid_lon, mesh=self._mesh)
        mesh_x, grid_x, edge_attr = get_bipartite_graph_spatial_features(
            senders_node_lat=self._mesh_nodes_lat, senders_node_lon=self._mesh_nodes_lon, receivers_node_lat=self._grid_nodes_lat,
            receivers_node_lon=self._grid_nodes_lon, senders=senders, receivers=receivers,
            edge_normalization_factor=self._mesh2grid_edge_normalization_factor)
        self.m2g_edges_dim = edge_attr.shape[1]
        g = HeteroData()
        g["mesh_nodes"].x = self._f32(mesh_x)
        g["grid_nodes"].x = self._f32(grid_x)
        g["mesh_nodes", "to", "grid_nodes"].edge_index = self._ix(senders, receivers)
        g["mesh_nodes", "to", "grid_nodes"].edge_attr = self._f32(edge_attr)
        return g

    def _init_khop_mesh_graph(self) -> Data:
        ei = self.mesh_graph.edge_index.cpu().numpy()
        khop = khop_edge_index(ei[0], ei[1], self._num_mesh_nodes, self.num_hops)
        graph = Data(x=self.mesh_graph.x, edge_index=torch.tensor(khop, dtype=torch.long, device=self.device))
        if self.add_edge_features_to_khop:  # (expensive on a big mesh: one rotation per edge)
            _, edge_attr = get_graph_spatial_features(node_lat=self._mesh_nodes_lat, node_lon=self._mesh_nodes_lon, senders=khop[0],
                                                      receivers=khop[1])
            graph.edge_attr = self._f32(edge_attr)
        return graph
