"""noize_job_amd -- MI355X-native (gfx950, hand-written HIP) engine for noize-job's per-cell
terrain path: fractal noise -> separable kernel filters -> flow map -> value erosion -> mesh.

Importing the package loads libnoize_hip.so through the C ABI of include/noize_hip.h and raises if
it is missing: there is no CPU or PyTorch fallback in the product path.
"""
from . import _native
from ._native import NoizeError, Stripe
from .runtime import Context, DeviceTile, JobHandle
from .pipeline import (BasePipeline, BlurHelper, ConstantOperationType, ConstantStage, CropStage, CurveStage, DepressionFillStage, DownsampleData, DrainageAreaStage, DownsampleStage, ErosionStage, FlowMapStage, FluvialErosionStage, FractalNoise, FractalShape, GaussSigma,
                       GeneratorData, GeneratorDataBatch, HydraulicBorder, HydraulicErosionStage, KernelFilterStage, KernelFilterType, MeshBuffers, MeshStageData,
                       MeshTileStage, MeshType, NoiseStage, PipelineJoint, PipelineStage, PipelineWorkItem, ReduceData,
                       ReducePipeline, ReduceStage, ShapedNoiseStage, UpsampleStage, Upstream, WarpedNoiseStage, WatershedStage,
                       ReductionType, ResampleFilter, StageGaussianBlur, StageThermalErosion,
                       StageIO, StageSmoothBlur, StreamOrderStage, ImplicitFluvialStage, HillslopeDiffusionStage, MfdDrainageStage, FlowRouting, MfdFluvialStage, SedimentFluvialStage)

from .pipeline_state import (HandleLock, MeshTileReferenceDataStage, PipelineStateManager, ReadGeneratorContextStage,
                             WriteGeneratorContextStage)

from .live_erosion import (ColorChannelByte, ErosionMode, ErosionSettings, ErosiveEvents, LiveErosion, ParticleQueue,
                           tile_set_meta)

__all__ = [n for n in dir() if not n.startswith("_")]
