"""graph_weather/models/gencast/graph/icosahedral_mesh.py of the reference."""
from graph_weather_amd.gencast_graphs import (  # noqa: F401
    TriangularMesh,
    faces_to_edges,
    get_hierarchy_of_triangular_meshes_for_sphere,
    get_icosahedron,
)
