"""BEVerse-named counterparts (mmdet3d/models/beverse/models/{basic,motion}_modules.py of the
reference tree): ``FuturePrediction``, ``ResFuturePrediction`` / ``V2`` / ``V1``, ``GRUCell``, ``SpatialDistributionModule``,
``DistributionModule`` — the class names BASELINE.json's north star lists.  Secondary, signature-compatible:
the shipped StreamingFlow evaluation never reaches them."""
from .motion_modules import (DistributionEncoder, DistributionModule, FuturePrediction, ResFuturePrediction,  # noqa: F401
                             ResFuturePredictionV1, ResFuturePredictionV2, SpatialDistributionModule, warp_with_flow)
from .basic_modules import Bottleneck, ConvBlock, GRUCell, SpatialGRU  # noqa: F401
