"""graph_weather_amd - MI355X (gfx950) native implementation of the GraphWeatherForecaster hot path.

Mirrors the import surface of the reference for that path (``graph_weather/__init__.py:9``,
``graph_weather/models/__init__.py:13-15``): ``GraphWeatherForecaster``, ``Encoder``, ``Processor``, ``Decoder``,
``GraphProcessor``, ``MLP``, ``NormalizedMSELoss``, ``AMSENormalizedLoss``.
"""
from .analysis import AssimilatorEncoder, GraphWeatherAssimilator, GraphWeatherAssimilatorConfig  # noqa: F401
from .forecast import GraphWeatherForecaster, GraphWeatherForecasterConfig  # noqa: F401
from .layers import (  # noqa: F401
    MLP,
    AssimilatorDecoder,
    Decoder,
    EdgeProcessor,
    Encoder,
    GraphProcessor,
    NodeProcessor,
    Processor,
    build_graph_processor_block,
    set_compute_dtype,
    set_deterministic,
)
from .ops import BF16X3  # noqa: F401  (set_compute_dtype(model, BF16X3): split-operand products, csrc/gw_split.hip)
from .graphcast import GraphCast, GraphCastConfig  # noqa: F401
from .losses import AMSENormalizedLoss, EnsembleCRPSLoss, NormalizedMSELoss  # noqa: F401  (AMSE: csrc/gw_sht.hip; CRPS: csrc/gw_crps.hip)
from .regional import (  # noqa: F401
    BoundaryNudgingLayer,
    DynamicGraphBuilder,
    RegionalForecaster,
    RegionalForecasterConfig,
)
from .constraint import PhysicalConstraintLayer  # noqa: F401  (csrc/gw_constraint.hip)
from .thermalizer import AdaptiveUNet, ThermalizerLayer  # noqa: F401  (csrc/gw_thermal.hip)
from .modulation import FiLMApplier, FiLMGenerator, StochasticDecompositionLayer  # noqa: F401  (csrc/gw_modulate.hip)
from .fengwu_ghr import ImageMetaModel, MetaModel, WrapperImageModel, WrapperMetaModel  # noqa: F401  (csrc/gw_fengwu.hip)
from .cafa import (  # noqa: F401  (csrc/gw_cafa.hip, axial addressing of csrc/gw_fengwu.hip)
    AxialAttention,
    CaFADecoder,
    CaFAEncoder,
    CaFAForecaster,
    CaFAProcessor,
    FactorizedAttention,
    FactorizedTransformerBlock,
)
from .aurora import (  # noqa: F401  (csrc/gw_aurora.hip, csrc/gw_conv3d.hip, masked attention of csrc/gw_fengwu.hip)
    AuroraModel,
    Decoder3D,
    EarthSystemLoss,
    PerceiverProcessor,
    PointCloudProcessor,
    PointDecoder,
    PointEncoder,
    ProcessorConfig,
    SelfAttentionLayer,
    Swin3DEncoder,
)
from . import gencast  # noqa: F401  (csrc/gw_gencast.hip; its Encoder / Processor / Decoder / MLP stay in the module: the names above are the forecaster's)
from . import gencast_graphs, gencast_model  # noqa: F401  (GenCast's GraphBuilder and Denoiser: batch-shared route of csrc/gw_gencast.hip)
from . import gencast_sparse  # noqa: F401  (GenCast's sparse processor blocks: the masked attention of csrc/gw_sparse_attn.hip)
from . import gencast_sampler  # noqa: F401  (GenCast's Sampler and WeightedMSELoss; the inverse transform of csrc/gw_sht.hip draws the noise)
from .gencast_sampler import Sampler, WeightedMSELoss  # noqa: F401
from .weathermesh import (  # noqa: F401  (WeatherMesh's processor: the 3-D neighbourhood attention of csrc/gw_na3d.hip)
    NeighborhoodAttention3D,
    WeatherMeshProcessor,
    WeatherMeshProcessorConfig,
)
from .weathermesh_model import (  # noqa: F401  (WeatherMesh's conv towers, encoder, decoder and model: csrc/gw_convnd.hip)
    ConvDownBlock,
    ConvUpBlock,
    WeatherMesh,
    WeatherMeshConfig,
    WeatherMeshDecoder,
    WeatherMeshDecoderConfig,
    WeatherMeshEncoder,
    WeatherMeshEncoderConfig,
    WeatherMeshOutput,
)
from .graphed import ForwardGraph  # noqa: F401  (the inference forward as one HIP graph)
from .rollout import rollout  # noqa: F401
from .optim import AdamW  # noqa: F401

__version__ = "0.1.0"
