"""graph_weather/models/weathermesh of the reference: the processor (``processor``), the convolution blocks (``layers``), the
encoder, the decoder and the model (``weathermesh2``).  The reference's own ``__init__.py`` is empty; the classes are exported here for convenience.  ``layers``, ``encoder``, ``decoder`` and ``weathermesh2`` are sub-package directories with one
re-export line each (the reference has modules): the import paths are the same."""
from .decoder import WeatherMeshDecoder, WeatherMeshDecoderConfig  # noqa: F401
from .encoder import WeatherMeshEncoder, WeatherMeshEncoderConfig  # noqa: F401
from .layers import ConvDownBlock, ConvUpBlock  # noqa: F401
from .processor import WeatherMeshProcessor, WeatherMeshProcessorConfig  # noqa: F401
from .weathermesh2 import WeatherMesh, WeatherMeshConfig, WeatherMeshOutput  # noqa: F401
