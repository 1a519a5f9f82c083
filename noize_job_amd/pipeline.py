"""Host-side mirror of the reference's Pipeline / PipelineStage operator API for the hot path.

Same names, field names, argument meaning and error behaviour as the C# classes, so that stage
graphs written against the reference (NoiseStage -> KernelFilterStage -> FlowMapStage ->
MeshTileStage ...) run unchanged; each `Schedule` body calls the C ABI where the reference calls a
Burst job delegate.  (The C# host in INTEGRATION.md is the same code in the reference's own
language; no .NET toolchain exists in this image, so the Python mirror is what the tests drive.)

Reference files: Pipeline/Stage/PipelineStage.cs, Pipeline/Stage/StageIO.cs,
Pipeline/Stage/StageIOTypes/*.cs, Pipeline/Stage/PipelineDefinition.cs,
Pipeline/Executable/Pipeline.cs, Noise/NoiseStage.cs, Filter/KernelFilterStage.cs,
Filter/Kernel/Blur/Stage{Gaussian,Smooth}Blur.cs, Geologic/Stage/FlowMapStage.cs,
Mesh/Stage/MeshTileStage.cs.
"""
import collections
import ctypes as C
import enum

import numpy as np

from . import _native as N
from .runtime import JobHandle


# ---- enums (values are the C# enum values) ----------------------------------------------------
class FractalNoise(enum.IntEnum):  # Noise/NoiseStage.cs:15-24
    Sin = 0
    Perlin = 1
    PeriodicPerlin = 2
    Simplex = 3
    RotatedSimplex = 4
    Cellular = 5
    DomainRotatedPerlin = 6
    DomainRotatedSimplex = 7


class FractalShape(enum.IntEnum):  # new-framework: the octave shape of ShapedNoiseStage (enum nz_fractal_shape)
    Fbm = 0
    Billow = 1
    Ridged = 2


class HydraulicBorder(enum.IntEnum):  # new-framework: the tile border of HydraulicErosionStage (enum nz_hydraulic_border)
    Closed = 0  # clamp to edge: no water and no sediment leave the tile
    Open = 1    # the tile is cut out of a larger world: water and sediment run off the map


class ResampleFilter(enum.IntEnum):  # new-framework: the filter of UpsampleStage (enum nz_resample_filter)
    Nearest = 0
    Bilinear = 1
    CatmullRom = 2


class KernelFilterType(enum.IntEnum):  # Filter/Kernel/KernelJob.cs:79-94
    Gauss9_S1 = 0
    Gauss7_S1 = 1
    Gauss5_S1 = 2
    Gauss3_S1 = 3
    Gauss9_S2 = 4
    Gauss7_S2 = 5
    Gauss5_S2 = 6
    Gauss3_S2 = 7
    Smooth3 = 8
    Sobel3Horizontal = 9
    Sobel3Vertical = 10
    Sobel3_2D = 11
    Prewitt3Horizontal = 12
    Prewitt3Vertical = 13


class GaussSigma(enum.IntEnum):  # Filter/Kernel/Blur/BlurKernels.cs:8-25; sigma = 0.5 * (value + 1)
    s0d50 = 0
    s1d00 = 1
    s1d50 = 2
    s2d00 = 3
    s2d50 = 4
    s3d00 = 5
    s3d50 = 6
    s4d00 = 7
    s4d50 = 8
    s5d00 = 9
    s5d50 = 10
    s6d00 = 11
    s6d50 = 12
    s7d00 = 13
    s7d50 = 14
    s8d00 = 15


class ConstantOperationType(enum.IntEnum):  # Filter/ConstantStage.cs:15-18
    MULTIPLY = 0
    BINARIZE = 1


class ReductionType(enum.IntEnum):  # Filter/Reduce/ReduceStage.cs:12-18
    SUBTRACT = 0
    MULTIPLY = 1
    ROOTSUMSQUARES = 2
    MAX = 3
    MIN = 4


class MeshType(enum.IntEnum):  # Mesh/Stage/MeshTileStage.cs:23-26
    SquareGridHeightMap = 0
    OvershootSquareGridHeightMap = 1


class BlurHelper:  # Filter/Kernel/Blur/BlurKernels.cs:27-37
    max_width = 25

    @staticmethod
    def limitWidth(width):
        if width % 2 == 0:
            width += 1
        width = min(width, BlurHelper.max_width)
        return max(3, width)


# ---- StageIO payloads ---------------------------------------------------------------------------
class StageIO:  # Pipeline/Stage/StageIO.cs:8-11
    def __init__(self, uuid="", data=None):
        self.uuid = uuid
        self.data = data  # DeviceTile (the NativeSlice<float>)


class GeneratorData(StageIO):  # StageIOTypes/GeneratorData.cs:9-15
    """`write` (optional, new-framework): a second plane of the same size, the WRITE slice of the tile's RWTileData
    pair (Pipeline/Tiles/TileData.cs:49-93).  With it the stencil stages (kernel filter, blurs, erosion, flow map)
    run their nz_*_rw forms: TileHelpers.SWAP_RWTILE is a swap of `data` and `write` instead of a flush copy, so
    after a stage `data` is whichever of the two planes holds the result."""

    def __init__(self, uuid="", data=None, resolution=512, xpos=0, zpos=0, write=None):
        super().__init__(uuid, data)
        self.resolution = resolution
        self.xpos = xpos
        self.zpos = zpos
        self.write = write


def _tiles_of(d):
    """The planes an element-wise / per-tile job has to visit: the payload's one plane, or every tile of a
    GeneratorDataBatch (those jobs take `resolution`, not a cell count, so a batch goes tile by tile)."""
    if isinstance(d, GeneratorDataBatch):
        return [d.tile(k) for k in range(d.count)]
    return [d.data]


def _call_rw(ctx, name, d, *args, dep=None):
    """Runs an nz_*_rw entry on the payload's READ / WRITE pair and adopts the pair as the call left it."""
    t = N.RWTile(d.data.ptr, d.write.ptr, d.resolution, getattr(d, "count", 1))
    handle = ctx.call(name, C.byref(t), *args, dep=dep)
    if t.read != d.data.ptr:
        d.data, d.write = d.write, d.data
    return handle


class GeneratorDataBatch(GeneratorData):
    """New-framework payload: `count` independent tiles of `resolution`^2 cells stored back to back in `data`
    (tile k at offset k * resolution^2), world positions in `positions` (device int32 array {xpos, zpos} per
    tile).  The noise / filter / blur / erosion / flow-map stages run such a batch through one launch
    sequence (nz_*_batch); every tile comes out exactly as it would alone."""

    def __init__(self, uuid="", data=None, resolution=512, positions=None, count=1, write=None, hostPositions=None):
        super().__init__(uuid, data, resolution, 0, 0, write)
        self.positions = positions
        self.count = count
        self.hostPositions = hostPositions  # the same pairs on the host (int32, count x 2), for a stage that rescales them

    @classmethod
    def create(cls, ctx, uuid, resolution, positions):
        """positions: sequence of (xpos, zpos); allocates the stacked planes and uploads the positions."""
        pos = np.ascontiguousarray(positions, np.int32).reshape(-1, 2)
        return cls(uuid, ctx.alloc(len(pos) * resolution * resolution), resolution, ctx.from_host(pos), len(pos),
                   hostPositions=pos)

    def tile(self, k):
        n = self.resolution * self.resolution
        return self.data.offset(k * n, n)


class MeshStageData(StageIO):  # StageIOTypes/MeshStageData.cs:9-21
    def __init__(self, uuid="", data=None, resolution=512, inputResolution=512, marginPix=5, tileSize=512.0,
                 tileHeight=512.0, xpos=0, zpos=0, mesh=None, count=1):
        super().__init__(uuid, data)
        self.count = count  # new-framework: `count` height planes stored back to back -> `count` meshes
        self.resolution = resolution
        self.inputResolution = inputResolution
        self.marginPix = marginPix
        self.tileSize = tileSize
        self.tileHeight = tileHeight
        self.xpos = xpos
        self.zpos = zpos
        self.mesh = mesh  # MeshBuffers, stands in for UnityEngine.Mesh


class ReduceData(StageIO):  # StageIOTypes/ReduceData.cs:9-17
    def __init__(self, uuid="", data=None, rightData=None, resolution=512, xpos=0, zpos=0):
        super().__init__(uuid, data)
        self.rightData = rightData
        self.resolution = resolution
        self.xpos = xpos
        self.zpos = zpos


class DownsampleData(StageIO):  # StageIOTypes/DownsampleData.cs:9-17
    def __init__(self, uuid="", data=None, inputData=None, resolution=512, inputResolution=512):
        super().__init__(uuid, data)
        self.inputData = inputData
        self.resolution = resolution
        self.inputResolution = inputResolution


class MeshBuffers:
    """What Mesh.AllocateWritableMeshData + PositionStream32.Setup provide (Mesh/Streams/
    PositionStream.cs:90-123): one interleaved 48-byte vertex stream and a uint32 index buffer."""
    VERTEX_DTYPE = np.dtype([("position", np.float32, 3), ("normal", np.float32, 3), ("tangent", np.float32, 4),
                             ("texCoord0", np.float32, 2)])

    def __init__(self):
        self.vertices = None  # DeviceTile, float32 view of the 48-byte records
        self.indices = None   # DeviceTile, uint32
        self.vertexCount = 0
        self.indexCount = 0

    def vertex_array(self):
        return self.vertices.ToArray().view(self.VERTEX_DTYPE).reshape(-1)

    def index_array(self):
        return self.indices.ToArray()


class PipelineWorkItem:  # Pipeline/Stage/PipelineDefinition.cs:18-25
    def __init__(self, data, completeAction=None, scheduledAction=None, dependency=None, stageManager=None):
        self.data = data
        self.completeAction = completeAction
        self.scheduledAction = scheduledAction
        self.dependency = dependency if dependency is not None else JobHandle()
        self.stageManager = stageManager


# ---- PipelineStage ------------------------------------------------------------------------------
class PipelineStage:  # Pipeline/Stage/PipelineStage.cs:10-62
    def __init__(self, ctx):
        self.ctx = ctx
        self.jobHandle = JobHandle()
        self.OnStageScheduledAction = []  # multicast delegate
        self.arraysInitialized = False
        self.dataLength = 0

    def ResizeNativeContainers(self, size):
        pass

    def IsSchedulable(self, job):
        return True

    def CheckRequirements(self, io_type, requirements):
        if isinstance(requirements.data, io_type):
            d = requirements.data
            if d.data.Length != self.dataLength:
                self.dataLength = d.data.Length
                self.ResizeNativeContainers(d.data.Length)
        else:
            raise Exception("Unhandled stageio %s" % type(requirements.data).__name__)

    def Schedule(self, requirements, dependency):
        pass

    def ReceiveHandledInput(self, requirements, dependency):
        self.Schedule(requirements, dependency)
        self.TransformData(requirements)
        self.OnStageScheduled(requirements, self.jobHandle)

    def Destroy(self):
        self.OnDestroy()

    def TransformData(self, data):
        pass

    def OnStageScheduled(self, requirements, dependency):
        for action in self.OnStageScheduledAction:
            action(requirements, self.jobHandle)

    def OnStageComplete(self):
        pass

    def OnDestroy(self):
        pass

    # helper shared by the stages that own one `tmp` plane (KernelFilterStage.cs:22-29 etc.)
    def _resize_tmp(self):
        if getattr(self, "tmp", None) is not None and self.tmp.IsCreated:
            self.tmp.Dispose()
        self.tmp = self.ctx.alloc(self.dataLength)


class NoiseStage(PipelineStage):  # Noise/NoiseStage.cs:13-61
    def __init__(self, ctx, noiseType=FractalNoise.Sin, hurst=0.0, startingAmplitude=1.0, octaves=1, stepdown=2.0,
                 detuneRate=0.0, noiseSize=1000):
        super().__init__(ctx)
        self.noiseType = noiseType
        self.hurst = hurst
        self.startingAmplitude = startingAmplitude
        self.octaves = octaves
        self.stepdown = stepdown
        self.detuneRate = detuneRate
        self.noiseSize = noiseSize

    def Schedule(self, requirements, dependency):
        self.CheckRequirements(GeneratorData, requirements)
        d = requirements.data
        if isinstance(d, GeneratorDataBatch):
            self.jobHandle = self.ctx.call("nz_fractal_batch", int(self.noiseType), d.data.ptr, d.resolution, d.count,
                                           d.positions.ptr, self.hurst, self.startingAmplitude, self.stepdown,
                                           self.detuneRate, self.octaves, self.noiseSize, dep=dependency)
            return
        # jobs[(int)noiseType](d.data, d.resolution, hurst, startingAmplitude, stepdown, detuneRate, octaves, ...)
        self.jobHandle = self.ctx.call("nz_fractal", int(self.noiseType), d.data.ptr, d.resolution, self.hurst,
                                       self.startingAmplitude, self.stepdown, self.detuneRate, self.octaves, d.xpos,
                                       d.zpos, self.noiseSize, dep=dependency)


class ShapedNoiseStage(NoiseStage):
    """New-framework: NoiseStage with an octave shape -- FractalShape.Billow (|2v - 1| per octave) or FractalShape.Ridged
    (Musgrave's ridged multifractal, (ridgeOffset - |2v - 1|)^2 weighted by the previous octave through ridgeGain).  Fbm
    gives the bits of NoiseStage.  A subclass, so the stock-list fast paths (exact type) never take it for plain fBm."""

    def __init__(self, ctx, noiseType=FractalNoise.Sin, hurst=0.0, startingAmplitude=1.0, octaves=1, stepdown=2.0,
                 detuneRate=0.0, noiseSize=1000, shape=FractalShape.Ridged, ridgeOffset=1.0, ridgeGain=2.0):
        super().__init__(ctx, noiseType, hurst, startingAmplitude, octaves, stepdown, detuneRate, noiseSize)
        self.shape = shape
        self.ridgeOffset = ridgeOffset
        self.ridgeGain = ridgeGain

    def Schedule(self, requirements, dependency):
        self.CheckRequirements(GeneratorData, requirements)
        d = requirements.data
        if isinstance(d, GeneratorDataBatch):
            self.jobHandle = self.ctx.call("nz_fractal_shaped_batch", int(self.noiseType), d.data.ptr, d.resolution,
                                           d.count, d.positions.ptr, self.hurst, self.startingAmplitude, self.stepdown,
                                           self.detuneRate, self.octaves, self.noiseSize, int(self.shape),
                                           self.ridgeOffset, self.ridgeGain, dep=dependency)
            return
        self.jobHandle = self.ctx.call("nz_fractal_shaped", int(self.noiseType), d.data.ptr, d.resolution, self.hurst,
                                       self.startingAmplitude, self.stepdown, self.detuneRate, self.octaves, d.xpos,
                                       d.zpos, self.noiseSize, int(self.shape), self.ridgeOffset, self.ridgeGain,
                                       dep=dependency)


class WarpedNoiseStage(ShapedNoiseStage):
    """New-framework: a ShapedNoiseStage read at domain-warped coordinates (Quilez's f(p + s q(p))): each cell moves by
    (2q - 1) warpStrength cells, q a plain fBm of the same basis over warpOctaves octaves at warpScale times the noise's
    frequency.  warpStrength 0 or warpOctaves 0 gives the bits of ShapedNoiseStage.  A subclass of NoiseStage, so the
    stock-list fast paths (exact type) never take it for plain fBm."""

    def __init__(self, ctx, noiseType=FractalNoise.Sin, hurst=0.0, startingAmplitude=1.0, octaves=1, stepdown=2.0,
                 detuneRate=0.0, noiseSize=1000, shape=FractalShape.Fbm, ridgeOffset=1.0, ridgeGain=2.0,
                 warpStrength=0.0, warpScale=1.0, warpOctaves=4):
        super().__init__(ctx, noiseType, hurst, startingAmplitude, octaves, stepdown, detuneRate, noiseSize, shape,
                         ridgeOffset, ridgeGain)
        self.warpStrength = warpStrength
        self.warpScale = warpScale
        self.warpOctaves = warpOctaves

    def Schedule(self, requirements, dependency):
        self.CheckRequirements(GeneratorData, requirements)
        d = requirements.data
        warp = (self.warpStrength, self.warpScale, self.warpOctaves)
        if isinstance(d, GeneratorDataBatch):
            self.jobHandle = self.ctx.call("nz_fractal_warped_batch", int(self.noiseType), d.data.ptr, d.resolution,
                                           d.count, d.positions.ptr, self.hurst, self.startingAmplitude, self.stepdown,
                                           self.detuneRate, self.octaves, self.noiseSize, int(self.shape),
                                           self.ridgeOffset, self.ridgeGain, *warp, dep=dependency)
            return
        self.jobHandle = self.ctx.call("nz_fractal_warped", int(self.noiseType), d.data.ptr, d.resolution, self.hurst,
                                       self.startingAmplitude, self.stepdown, self.detuneRate, self.octaves, d.xpos,
                                       d.zpos, self.noiseSize, int(self.shape), self.ridgeOffset, self.ridgeGain, *warp,
                                       dep=dependency)


class KernelFilterStage(PipelineStage):  # Filter/KernelFilterStage.cs:13-51
    def __init__(self, ctx, filter=KernelFilterType.Gauss9_S1, iterations=1):
        super().__init__(ctx)
        self.filter = filter
        self.iterations = iterations
        self.tmp = None

    def ResizeNativeContainers(self, size):
        self._resize_tmp()

    def Schedule(self, requirements, dependency):
        self.CheckRequirements(GeneratorData, requirements)
        d = requirements.data
        if d.write is not None and self.filter != KernelFilterType.Sobel3_2D:
            self.jobHandle = _call_rw(self.ctx, "nz_kernel_filter_stage_rw", d, int(self.filter), self.iterations,
                                      dep=dependency)
            return
        if isinstance(d, GeneratorDataBatch):
            self.jobHandle = self.ctx.call("nz_kernel_filter_stage_batch", d.data.ptr, self.tmp.ptr, int(self.filter),
                                           self.iterations, d.resolution, d.count, dep=dependency)
            return
        # the reference chains `iterations` SeparableKernelFilter.Schedule calls (:35-41); the
        # library fuses the chain into as few launches as halo growth allows
        self.jobHandle = self.ctx.call("nz_kernel_filter_stage", d.data.ptr, self.tmp.ptr, int(self.filter),
                                       self.iterations, d.resolution, dep=dependency)

    def OnDestroy(self):
        if self.tmp is not None and self.tmp.IsCreated:
            self.tmp.Dispose()


class StageGaussianBlur(PipelineStage):  # Filter/Kernel/Blur/StageGaussianBlur.cs:14-53
    def __init__(self, ctx, iterations=1, sigma=GaussSigma.s0d50, width=3):
        super().__init__(ctx)
        self.iterations = iterations
        self.sigma = sigma
        self.width = width
        self.tmp = None

    def ResizeNativeContainers(self, size):
        self._resize_tmp()

    def Schedule(self, requirements, dependency):
        self.CheckRequirements(GeneratorData, requirements)
        d = requirements.data
        width_ = BlurHelper.limitWidth(self.width)
        if d.write is not None:
            self.jobHandle = _call_rw(self.ctx, "nz_gauss_blur_stage_rw", d, width_, int(self.sigma), self.iterations,
                                      dep=dependency)
            return
        if isinstance(d, GeneratorDataBatch):
            self.jobHandle = self.ctx.call("nz_gauss_blur_stage_batch", d.data.ptr, self.tmp.ptr, width_, int(self.sigma),
                                           self.iterations, d.resolution, d.count, dep=dependency)
            return
        self.jobHandle = self.ctx.call("nz_gauss_blur_stage", d.data.ptr, self.tmp.ptr, width_, int(self.sigma),
                                       self.iterations, d.resolution, dep=dependency)

    def OnDestroy(self):
        if self.tmp is not None and self.tmp.IsCreated:
            self.tmp.Dispose()


class StageSmoothBlur(PipelineStage):  # Filter/Kernel/Blur/StageSmoothBlur.cs:14-52
    def __init__(self, ctx, iterations=1, width=1):
        super().__init__(ctx)
        self.iterations = iterations
        self.width = width
        self.tmp = None

    def ResizeNativeContainers(self, size):
        self._resize_tmp()

    def Schedule(self, requirements, dependency):
        self.CheckRequirements(GeneratorData, requirements)
        d = requirements.data
        width_ = BlurHelper.limitWidth(self.width)
        if d.write is not None:  # a batch too: the _rw entries honour nz_rw_tile.count
            self.jobHandle = _call_rw(self.ctx, "nz_smooth_blur_stage_rw", d, width_, self.iterations, dep=dependency)
            return
        if isinstance(d, GeneratorDataBatch):
            self.jobHandle = self.ctx.call("nz_smooth_blur_stage_batch", d.data.ptr, self.tmp.ptr, width_,
                                           self.iterations, d.resolution, d.count, dep=dependency)
            return
        self.jobHandle = self.ctx.call("nz_smooth_blur_stage", d.data.ptr, self.tmp.ptr, width_, self.iterations,
                                       d.resolution, dep=dependency)

    def OnDestroy(self):
        if self.tmp is not None and self.tmp.IsCreated:
            self.tmp.Dispose()


class ErosionStage(PipelineStage):
    """ErosionKernelJob (Filter/Kernel/KernelJob.cs:317-350) has no PipelineStage wrapper in the
    reference; this stage applies its delegate `iterations` times in KernelFilterStage's shape."""

    def __init__(self, ctx, iterations=1):
        super().__init__(ctx)
        self.iterations = iterations
        self.tmp = None

    def ResizeNativeContainers(self, size):
        self._resize_tmp()

    def Schedule(self, requirements, dependency):
        self.CheckRequirements(GeneratorData, requirements)
        d = requirements.data
        if d.write is not None:
            self.jobHandle = _call_rw(self.ctx, "nz_erosion_stage_rw", d, self.iterations, dep=dependency)
            return
        if isinstance(d, GeneratorDataBatch):
            self.jobHandle = self.ctx.call("nz_erosion_stage_batch", d.data.ptr, self.tmp.ptr, self.iterations,
                                           d.resolution, d.count, dep=dependency)
            return
        self.jobHandle = self.ctx.call("nz_erosion_stage", d.data.ptr, self.tmp.ptr, self.iterations, d.resolution,
                                       dep=dependency)

    def OnDestroy(self):
        if self.tmp is not None and self.tmp.IsCreated:
            self.tmp.Dispose()


class ConstantStage(PipelineStage):  # Filter/ConstantStage.cs:13-56
    def __init__(self, ctx, operation=ConstantOperationType.MULTIPLY, value=0.5):
        super().__init__(ctx)
        self.operation = operation
        self.value = value
        self.tmp = None

    def ResizeNativeContainers(self, size):
        self._resize_tmp()

    def Schedule(self, requirements, dependency):
        self.CheckRequirements(GeneratorData, requirements)
        d = requirements.data
        for t in _tiles_of(d):
            self.jobHandle = dependency = self.ctx.call("nz_constant_job", int(self.operation), t.ptr, self.tmp.ptr,
                                                        self.value, d.resolution, dep=dependency)

    def OnDestroy(self):
        if self.tmp is not None and self.tmp.IsCreated:
            self.tmp.Dispose()


class ReduceStage(PipelineStage):  # Filter/Reduce/ReduceStage.cs:20-69
    def __init__(self, ctx, operation=ReductionType.SUBTRACT):
        super().__init__(ctx)
        self.operation = operation
        self.tmp = None

    def ResizeNativeContainers(self, size):
        self._resize_tmp()

    def Schedule(self, requirements, dependency):
        self.CheckRequirements(ReduceData, requirements)
        d = requirements.data
        self.jobHandle = self.ctx.call("nz_reduction_job", int(self.operation), d.data.ptr, d.rightData.ptr,
                                       self.tmp.ptr, d.resolution, dep=dependency)

    def TransformData(self, inputData):  # :53-62: downstream stages see a GeneratorData
        d = inputData.data
        inputData.data = GeneratorData(d.uuid, d.data, d.resolution, d.xpos, d.zpos)

    def OnDestroy(self):
        if self.tmp is not None and self.tmp.IsCreated:
            self.tmp.Dispose()


class CurveStage(PipelineStage):  # Filter/Curve/CurveStage.cs:13-71
    """`unityCurve` is any callable t in [0,1) -> value (stands in for UnityEngine.AnimationCurve.Evaluate)."""

    def __init__(self, ctx, unityCurve=None, samples=256):
        super().__init__(ctx)
        self.unityCurve = unityCurve if unityCurve is not None else (lambda t: t)
        self.samples = samples
        self.curve = None
        self.tmp = None

    def ExtractCurve(self):  # :32-40
        host = np.array([self.unityCurve(np.float32(i) / np.float32(self.samples)) for i in range(self.samples)],
                        np.float32)
        if self.curve is None or not self.curve.IsCreated:
            self.curve = self.ctx.alloc(self.samples)
        self.curve.CopyFrom(host)
        return host

    def ResizeNativeContainers(self, size):
        if self.curve is not None and self.curve.IsCreated:
            self.curve.Dispose()
        self.curve = None
        self.ExtractCurve()
        self._resize_tmp()

    def Schedule(self, requirements, dependency):
        self.CheckRequirements(GeneratorData, requirements)
        d = requirements.data
        for t in _tiles_of(d):
            self.jobHandle = dependency = self.ctx.call("nz_curve_job", t.ptr, self.tmp.ptr, self.curve.ptr,
                                                        self.samples, d.resolution, dep=dependency)

    def OnDestroy(self):
        for t in (self.curve, self.tmp):
            if t is not None and t.IsCreated:
                t.Dispose()
        self.curve = self.tmp = None


class CropStage(PipelineStage):  # Filter/Sample/CropStage.cs:11-19
    """"CenterCropResolution" in the reference's menu; its job never sets the offset, so the crop is the
    top-left corner (Filter/Sample/CropJob.cs:43-59) -- reproduced as is."""

    def Schedule(self, requirements, dependency):
        d = requirements.data  # (DownsampleData) cast
        if not isinstance(d, DownsampleData):
            raise Exception("Unhandled stageio %s" % type(d).__name__)
        self.jobHandle = self.ctx.call("nz_crop_job", d.inputData.ptr, d.inputResolution, d.data.ptr, d.resolution,
                                       dep=dependency)


class _ResampleStage(PipelineStage):
    """What UpsampleStage and DownsampleStage share: the stage owns its output plane (resized when the input size changes)
    and hands downstream a GeneratorData -- or GeneratorDataBatch -- of the new resolution whose plane it is, as
    ReduceStage.TransformData hands on a GeneratorData."""

    def __init__(self, ctx, factor):
        super().__init__(ctx)
        self.factor = factor
        self.out = None
        self.outPositions = self.outHostPositions = None

    def _out_length(self, size):
        raise NotImplementedError

    def _out_position(self, v):
        raise NotImplementedError

    def ResizeNativeContainers(self, size):
        if self.out is not None and self.out.IsCreated:
            self.out.Dispose()
        self.out = self.ctx.alloc(self._out_length(size))

    def TransformData(self, inputData):
        d = inputData.data
        res = self._out_position(d.resolution)  # a resolution scales as a position does
        if isinstance(d, GeneratorDataBatch):
            # the positions are rescaled on the host from the payload's host copy (GeneratorDataBatch.create keeps one): no
            # wait on the device in the scheduling path, and one upload per new set of positions.  A payload built without
            # a host copy is read back once
            pos = d.hostPositions if d.hostPositions is not None else d.positions.ToArray()
            pos = np.array([self._out_position(int(v)) for v in np.asarray(pos).reshape(-1)], np.int32).reshape(-1, 2)
            if self.outHostPositions is None or not np.array_equal(pos, self.outHostPositions):
                if self.outPositions is not None and self.outPositions.IsCreated:
                    self.outPositions.Dispose()
                self.outPositions, self.outHostPositions = self.ctx.from_host(pos), pos
            inputData.data = GeneratorDataBatch(d.uuid, self.out, res, self.outPositions, d.count, hostPositions=pos)
        else:
            inputData.data = GeneratorData(d.uuid, self.out, res, self._out_position(d.xpos), self._out_position(d.zpos))

    def OnDestroy(self):
        for t in (self.out, self.outPositions):
            if t is not None and t.IsCreated:
                t.Dispose()
        self.out = self.outPositions = self.outHostPositions = None


class UpsampleStage(_ResampleStage):
    """New-framework stage: resolution R -> R * factor (2, 4 or 8) with nz_upsample: cell-centred nearest, bilinear or
    Catmull-Rom (include/noize_hip.h).  `base` (optional): a DeviceTile of the OUTPUT's size -- one tile, or `count` tiles
    for a batch -- that is added to the upsampled plane: the detail-transfer step of a coarse-to-fine pass.  xpos / zpos
    are multiplied by the factor."""

    def __init__(self, ctx, factor=2, filter=ResampleFilter.CatmullRom, base=None):
        super().__init__(ctx, factor)
        self.filter = filter
        self.base = base

    def _out_length(self, size):
        return size * self.factor * self.factor

    def _out_position(self, v):
        return v * self.factor

    def Schedule(self, requirements, dependency):
        self.CheckRequirements(GeneratorData, requirements)
        d = requirements.data
        base = self.base.ptr if self.base is not None else None
        if isinstance(d, GeneratorDataBatch):
            self.jobHandle = self.ctx.call("nz_upsample_batch", d.data.ptr, d.resolution, self.out.ptr, self.factor,
                                           int(self.filter), base, d.count, dep=dependency)
            return
        self.jobHandle = self.ctx.call("nz_upsample", d.data.ptr, d.resolution, self.out.ptr, self.factor, int(self.filter),
                                       base, dep=dependency)


class DownsampleStage(_ResampleStage):
    """New-framework stage: resolution R -> R / factor (2, 4 or 8; the factor divides R) with nz_downsample, the mean of
    every factor x factor block.  xpos / zpos are floor-divided by the factor."""

    def __init__(self, ctx, factor=2):
        super().__init__(ctx, factor)

    def _out_length(self, size):
        return size // (self.factor * self.factor)

    def _out_position(self, v):
        return v // self.factor

    def Schedule(self, requirements, dependency):
        self.CheckRequirements(GeneratorData, requirements)
        d = requirements.data
        if isinstance(d, GeneratorDataBatch):
            self.jobHandle = self.ctx.call("nz_downsample_batch", d.data.ptr, d.resolution, self.out.ptr, self.factor,
                                           d.count, dep=dependency)
            return
        self.jobHandle = self.ctx.call("nz_downsample", d.data.ptr, d.resolution, self.out.ptr, self.factor, dep=dependency)


class StageThermalErosion(PipelineStage):  # Filter/Kernel/Blur/StageThermalErosion.cs:12-29
    def __init__(self, ctx, iterations=1, talus=45, increment=0.5, meshHeightWidthRatio=0.75):
        super().__init__(ctx)
        self.iterations = iterations
        self.talus = talus
        self.increment = increment
        self.meshHeightWidthRatio = meshHeightWidthRatio

    def Schedule(self, requirements, dependency):
        self.CheckRequirements(GeneratorData, requirements)
        d = requirements.data
        for t in _tiles_of(d):
            self.jobHandle = dependency = self.ctx.call("nz_thermal_erosion", t.ptr, float(self.talus), self.increment,
                                                        self.meshHeightWidthRatio, self.iterations, d.resolution,
                                                        dep=dependency)


class FlowMapStage(PipelineStage):  # Geologic/Stage/FlowMapStage.cs:16-220
    def __init__(self, ctx, iterations=5, normMin=-0.1, normMax=0.1):
        super().__init__(ctx)
        self.iterations = iterations
        self.normMin = normMin
        self.normMax = normMax
        self.resolution = 0
        self.work = None  # the stage's water/flux READ+WRITE planes (:52-62)

    def DisposeArrays(self):
        if self.work is not None and self.work.IsCreated:
            self.work.Dispose()
        self.work = None

    def ResizeNativeContainers(self, size):
        self.DisposeArrays()
        # 11 planes per tile (nz_flowmap_stage_work_floats); a batch stacks its tiles inside every plane
        self.work = self.ctx.alloc(11 * self.dataLength)

    def Schedule(self, requirements, dependency):
        d = requirements.data
        if not isinstance(d, GeneratorData):
            raise Exception("Unhandled stageio %s" % type(d).__name__)
        if self.resolution != d.resolution:
            self.resolution = d.resolution
        self.CheckRequirements(GeneratorData, requirements)
        if d.write is not None:
            self.jobHandle = _call_rw(self.ctx, "nz_flowmap_stage_rw", d, self.work.ptr, self.iterations, self.normMin,
                                      self.normMax, dep=dependency)
            return
        if isinstance(d, GeneratorDataBatch):
            self.jobHandle = self.ctx.call("nz_flowmap_stage_batch", d.data.ptr, self.work.ptr, self.iterations,
                                           self.normMin, self.normMax, d.resolution, d.count, dep=dependency)
            return
        self.jobHandle = self.ctx.call("nz_flowmap_stage", d.data.ptr, self.work.ptr, self.iterations, self.normMin,
                                       self.normMax, d.resolution, dep=dependency)

    def OnDestroy(self):
        self.DisposeArrays()


class HydraulicErosionStage(PipelineStage):
    """Grid hydraulic erosion with sediment transport (new-framework feature; the model is the comment block of
    nz_hydraulic_erosion_stage in include/noize_hip.h): carves channels where water runs fast and steep and fills hollows
    where it slows.  Like FlowMapStage it owns its work planes; after the stage's handle completes, `water` holds the final
    water depth (a river and lake mask) of the last payload, `count` tiles of resolution^2 cells.

    border=Open lets water and sediment run off the tile.  rainMap / hardness: device planes of the payload's size
    (count * resolution^2 floats) the caller supplies and keeps alive -- rain is multiplied by rainMap, dissolve by
    1 - hardness.  recordMasks: the stage also owns `wear` and `deposits`, what every cell lost and what was laid down on
    it (result = input - wear + deposits up to rounding).  With all four at their defaults the stage calls the plain
    entries."""

    def __init__(self, ctx, iterations=200, initialWater=1e-4, rain=1e-4, evaporation=0.01, capacity=1.0, dissolve=0.3,
                 deposit=0.3, minTilt=0.01, border=HydraulicBorder.Closed, rainMap=None, hardness=None, recordMasks=False):
        super().__init__(ctx)
        self.iterations = iterations
        self.initialWater = initialWater
        self.rain = rain
        self.evaporation = evaporation
        self.capacity = capacity
        self.dissolve = dissolve
        self.deposit = deposit
        self.minTilt = minTilt
        self.border = border
        self.rainMap = rainMap
        self.hardness = hardness
        self.recordMasks = recordMasks
        self.resolution = 0
        self.count = 0
        self.work = None  # nz_hydraulic_erosion_work_floats planes; the first count * resolution^2 floats: the water
        self.masks = None  # recordMasks: wear, then deposits, count * resolution^2 floats each

    def DisposeArrays(self):
        for t in (self.work, self.masks):
            if t is not None and t.IsCreated:
                t.Dispose()
        self.work = self.masks = None

    def ResizeNativeContainers(self, size):
        self.DisposeArrays()
        self.work = self.ctx.alloc(N.lib.nz_hydraulic_erosion_work_floats(self.resolution, self.count))
        if self.recordMasks:
            self.masks = self.ctx.alloc(2 * self.count * self.resolution * self.resolution)

    def _params(self):
        return (self.iterations, self.initialWater, self.rain, self.evaporation, self.capacity, self.dissolve, self.deposit,
                self.minTilt)

    @property
    def water(self):
        """The water plane(s) of the last run: a view of the first count * resolution^2 floats of the work planes."""
        return self.work.offset(0, self.count * self.resolution * self.resolution)

    @property
    def wear(self):
        """recordMasks: what every cell of the last run lost to erosion (count * resolution^2 floats)."""
        n = self.count * self.resolution * self.resolution
        return self.masks.offset(0, n) if self.masks is not None else None

    @property
    def deposits(self):
        """recordMasks: what was laid down on every cell of the last run, the settled sediment included."""
        n = self.count * self.resolution * self.resolution
        return self.masks.offset(n, n) if self.masks is not None else None

    def _desc(self):
        """The nz_hydraulic_desc of the extended entries, or None when every option is at its default."""
        if not self.recordMasks and self.masks is not None:  # (switched off after a payload: wear and deposits are empty again)
            if self.masks.IsCreated:
                self.masks.Dispose()
            self.masks = None
        if (int(self.border) == HydraulicBorder.Closed and self.rainMap is None and self.hardness is None
                and not self.recordMasks):
            return None
        n = self.count * self.resolution * self.resolution
        for name, m in (("rainMap", self.rainMap), ("hardness", self.hardness)):
            if m is not None and m.Length != n:
                raise ValueError("HydraulicErosionStage.%s holds %d floats, the payload %d" % (name, m.Length, n))
        if self.recordMasks and (self.masks is None or self.masks.Length != 2 * n):  # (switched on after the first payload)
            self.ResizeNativeContainers(n)
        ptr = lambda t: t.ptr if t is not None else None  # noqa: E731
        return N.HydraulicDesc(*self._params(), int(self.border), ptr(self.rainMap), ptr(self.hardness), ptr(self.wear),
                               ptr(self.deposits))

    def Schedule(self, requirements, dependency):
        d = requirements.data
        if not isinstance(d, GeneratorData):
            raise Exception("Unhandled stageio %s" % type(d).__name__)
        # the work planes are sized on the payload's cell count (count * resolution^2), as CheckRequirements tracks it
        self.resolution, self.count = d.resolution, getattr(d, "count", 1)
        self.CheckRequirements(GeneratorData, requirements)
        desc = self._desc()  # raises before any launch when a map does not fit the payload
        if desc is not None:
            if d.write is not None:
                self.jobHandle = _call_rw(self.ctx, "nz_hydraulic_erosion_ex_rw", d, self.work.ptr, C.byref(desc),
                                          dep=dependency)
            elif isinstance(d, GeneratorDataBatch):
                self.jobHandle = self.ctx.call("nz_hydraulic_erosion_ex_batch", d.data.ptr, self.work.ptr, C.byref(desc),
                                               d.resolution, d.count, dep=dependency)
            else:
                self.jobHandle = self.ctx.call("nz_hydraulic_erosion_ex", d.data.ptr, self.work.ptr, C.byref(desc),
                                               d.resolution, dep=dependency)
            return
        if d.write is not None:
            self.jobHandle = _call_rw(self.ctx, "nz_hydraulic_erosion_stage_rw", d, self.work.ptr, *self._params(),
                                      dep=dependency)
            return
        if isinstance(d, GeneratorDataBatch):
            self.jobHandle = self.ctx.call("nz_hydraulic_erosion_stage_batch", d.data.ptr, self.work.ptr, *self._params(),
                                           d.resolution, d.count, dep=dependency)
            return
        self.jobHandle = self.ctx.call("nz_hydraulic_erosion_stage", d.data.ptr, self.work.ptr, *self._params(),
                                       d.resolution, dep=dependency)

    def OnDestroy(self):
        self.DisposeArrays()


class FluvialErosionStage(PipelineStage):
    """Stream-power fluvial erosion with drainage area (new-framework feature; the model is the comment block of
    nz_fluvial_erosion in include/noize_hip.h): every cell drains to its steepest-descent neighbour, the drainage area is
    accumulated down that tree and the bed is lowered by erodibility * sqrt(area) * slope against the uplift -- dendritic
    valleys that run from the ridges to the tile's border.  Like HydraulicErosionStage it owns its work planes; after the
    stage's handle completes, `drainage` holds the drainage area (the river map) of the last payload, `count` tiles of
    resolution^2 cells.

    seaLevel: cells at or below it are outlets like the border cells (the default, -FLT_MAX, switches it off).  rainMap /
    hardness / upliftMap / drainageIn: device planes of the payload's size (count * resolution^2 floats) the caller supplies
    and keeps alive -- rain is multiplied by rainMap, erodibility by 1 - hardness, uplift by upliftMap, and drainageIn is
    the drainage the accumulation starts from (the `drainage` of an earlier run, copied: it may not be the stage's own
    plane)."""

    SEA_OFF = -3.4028234663852886e38  # -FLT_MAX

    def __init__(self, ctx, iterations=200, erodibility=0.05, uplift=0.002, dt=1.0, rain=1.0, seaLevel=SEA_OFF,
                 rainMap=None, hardness=None, upliftMap=None, drainageIn=None):
        super().__init__(ctx)
        self.iterations = iterations
        self.erodibility = erodibility
        self.uplift = uplift
        self.dt = dt
        self.rain = rain
        self.seaLevel = seaLevel
        self.rainMap = rainMap
        self.hardness = hardness
        self.upliftMap = upliftMap
        self.drainageIn = drainageIn
        self.resolution = 0
        self.count = 0
        self.work = None  # nz_fluvial_erosion_work_floats planes; the first count * resolution^2 floats: the drainage

    def DisposeArrays(self):
        if self.work is not None and self.work.IsCreated:
            self.work.Dispose()
        self.work = None

    def ResizeNativeContainers(self, size):
        self.DisposeArrays()
        self.work = self.ctx.alloc(N.lib.nz_fluvial_erosion_work_floats(self.resolution, self.count))

    @property
    def drainage(self):
        """The drainage plane(s) of the last run: a view of the first count * resolution^2 floats of the work planes; None
        before the first payload and after OnDestroy."""
        if self.work is None:
            return None
        return self.work.offset(0, self.count * self.resolution * self.resolution)

    def _desc(self):
        n = self.count * self.resolution * self.resolution
        planes = (("rainMap", self.rainMap), ("hardness", self.hardness), ("upliftMap", self.upliftMap),
                  ("drainageIn", self.drainageIn))
        for name, m in planes:
            if m is not None and m.Length != n:
                raise ValueError("FluvialErosionStage.%s holds %d floats, the payload %d" % (name, m.Length, n))
        return N.FluvialDesc(self.iterations, self.erodibility, self.uplift, self.dt, self.rain, self.seaLevel,
                             *[m.ptr if m is not None else None for _, m in planes])

    def Schedule(self, requirements, dependency):
        d = requirements.data
        if not isinstance(d, GeneratorData):
            raise Exception("Unhandled stageio %s" % type(d).__name__)
        # the work planes are sized on the payload's cell count (count * resolution^2), as CheckRequirements tracks it
        self.resolution, self.count = d.resolution, getattr(d, "count", 1)
        self.CheckRequirements(GeneratorData, requirements)
        desc = self._desc()  # raises before any launch when a plane does not fit the payload
        if d.write is not None:
            self.jobHandle = _call_rw(self.ctx, "nz_fluvial_erosion_rw", d, self.work.ptr, C.byref(desc), dep=dependency)
        elif isinstance(d, GeneratorDataBatch):
            self.jobHandle = self.ctx.call("nz_fluvial_erosion_batch", d.data.ptr, self.work.ptr, C.byref(desc),
                                           d.resolution, d.count, dep=dependency)
        else:
            self.jobHandle = self.ctx.call("nz_fluvial_erosion", d.data.ptr, self.work.ptr, C.byref(desc), d.resolution,
                                           dep=dependency)

    def OnDestroy(self):
        self.DisposeArrays()


class DepressionFillStage(PipelineStage):
    """Depression filling (new-framework feature; the model is the comment block of nz_fill_depressions in
    include/noize_hip.h): every closed hollow is raised to its spill level plus an epsilon gradient, so that every cell but
    the outlets has a strictly lower neighbour and FluvialErosionStage's river network reaches the border from its first
    iteration.  Like FluvialErosionStage it owns its work planes.  With recordDepth, `depth` holds the lake depth of the
    last payload (filled surface minus bed, count * resolution^2 floats; zero where nothing was filled) once the stage's
    handle completes; `passes` and `converged` are the status words of that run.

    seaLevel: cells at or below it are outlets like the border cells (the default, -FLT_MAX, switches it off).  maxPasses:
    the number of pass launches; None means 64 + resolution // 4.  A budget that runs out is no error: converged is False,
    the heights are as they were and the depth is zero."""

    SEA_OFF = -3.4028234663852886e38  # -FLT_MAX

    def __init__(self, ctx, epsilon=1e-4, seaLevel=SEA_OFF, maxPasses=None, recordDepth=False):
        super().__init__(ctx)
        self.epsilon = epsilon
        self.seaLevel = seaLevel
        self.maxPasses = maxPasses
        self.recordDepth = recordDepth
        self.resolution = 0
        self.count = 0
        self.work = None    # nz_fill_depressions_work_floats floats; its first two int32: {passes, converged}
        self._depth = None  # the lake-depth planes (recordDepth)

    def DisposeArrays(self):
        for t in (self.work, self._depth):
            if t is not None and t.IsCreated:
                t.Dispose()
        self.work = self._depth = None

    def _size_work(self):
        """The work planes are sized on (resolution, count) -- the per-tile bytes depend on the number of 64 x 16 tiles --
        and not on the payload's cell count alone, which is all CheckRequirements tracks: two payloads of equal length can
        need different sizes."""
        need = N.lib.nz_fill_depressions_work_floats(self.resolution, self.count)
        if self.work is None or self.work.Length != need:
            if self.work is not None and self.work.IsCreated:
                self.work.Dispose()
            self.work = self.ctx.alloc(need)

    @property
    def depth(self):
        """The lake-depth plane(s) of the last run, or None: without recordDepth, before the first payload and after
        OnDestroy."""
        return self._depth

    def _status(self):
        if self.work is None:
            return None
        self.jobHandle.Complete()
        return self.ctx.wrap(self.work.ptr, 2, dtype=np.int32).ToArray()

    @property
    def passes(self):
        """Passes of the last run that did work (the launches after them returned at once); None before the first run."""
        s = self._status()
        return None if s is None else int(s[0])

    @property
    def converged(self):
        """Whether the last run reached the fixed point within maxPasses; None before the first run."""
        s = self._status()
        return None if s is None else bool(s[1])

    def Schedule(self, requirements, dependency):
        d = requirements.data
        if not isinstance(d, GeneratorData):
            raise Exception("Unhandled stageio %s" % type(d).__name__)
        self.resolution, self.count = d.resolution, getattr(d, "count", 1)
        self.CheckRequirements(GeneratorData, requirements)
        self._size_work()
        n = self.count * self.resolution * self.resolution
        if not self.recordDepth and self._depth is not None:
            self._depth.Dispose()
            self._depth = None
        if self.recordDepth and (self._depth is None or self._depth.Length != n):
            if self._depth is not None:
                self._depth.Dispose()
            self._depth = self.ctx.alloc(n)
        budget = self.maxPasses if self.maxPasses is not None else 64 + self.resolution // 4
        desc = N.FillDesc(self.epsilon, self.seaLevel, budget, self._depth.ptr if self._depth is not None else None)
        if d.write is not None:
            self.jobHandle = _call_rw(self.ctx, "nz_fill_depressions_rw", d, self.work.ptr, C.byref(desc), dep=dependency)
        elif isinstance(d, GeneratorDataBatch):
            self.jobHandle = self.ctx.call("nz_fill_depressions_batch", d.data.ptr, self.work.ptr, C.byref(desc),
                                           d.resolution, d.count, dep=dependency)
        else:
            self.jobHandle = self.ctx.call("nz_fill_depressions", d.data.ptr, self.work.ptr, C.byref(desc), d.resolution,
                                           dep=dependency)

    def OnDestroy(self):
        self.DisposeArrays()


class DrainageAreaStage(PipelineStage):
    """Drainage area (new-framework feature; the model is the comment block of nz_drainage_area in include/noize_hip.h): the
    exact flow accumulation over the steepest-descent tree of the payload's heights -- the river map -- in one call.  The
    heights pass through untouched.  Once the stage's handle completes, `drainage` holds the plane of the last payload
    (count * resolution^2 floats); `passes` and `converged` are the status words of that run.  Behind DepressionFillStage
    every river reaches the border, and the plane is what FluvialErosionStage(drainageIn=...) takes as a warm start.

    seaLevel: cells at or below it are outlets like the border cells (the default, -FLT_MAX, switches it off).  rainMap: a
    device plane of the payload's size the caller supplies and keeps alive; rain is multiplied by it.  maxPasses: the number
    of pass launches; None means 64 + resolution // 4.  A budget that runs out is no error: converged is False and the
    drainage is the start state, rain (times rainMap) in every cell.  out: a caller-supplied plane of the payload's size
    that receives the drainage; without it the stage owns the plane."""

    SEA_OFF = -3.4028234663852886e38  # -FLT_MAX
    _ENTRIES = ("nz_drainage_area", "nz_drainage_area_batch", "nz_drainage_area_work_floats")  # MfdDrainageStage has its own

    def __init__(self, ctx, rain=1.0, seaLevel=SEA_OFF, maxPasses=None, rainMap=None, out=None):
        super().__init__(ctx)
        self.rain = rain
        self.seaLevel = seaLevel
        self.maxPasses = maxPasses
        self.rainMap = rainMap
        self.out = out
        self.resolution = 0
        self.count = 0
        self.work = None    # nz_drainage_area_work_floats floats; its first two int32: {passes, converged}
        self._plane = None  # the stage's own drainage plane (no `out`)

    def _desc(self, rainMap):
        """The entry's descriptor for the current payload (MfdDrainageStage has its own)."""
        budget = self.maxPasses if self.maxPasses is not None else 64 + self.resolution // 4
        return N.DrainageDesc(self.rain, self.seaLevel, budget, rainMap)

    def DisposeArrays(self):
        for t in (self.work, self._plane):
            if t is not None and t.IsCreated:
                t.Dispose()
        self.work = self._plane = None

    @property
    def drainage(self):
        """The drainage plane(s) of the last run -- `out` when the caller gave one -- or None before the first payload and
        after OnDestroy."""
        if self.work is None:
            return None
        return self.out if self.out is not None else self._plane

    def _status(self):
        if self.work is None:
            return None
        self.jobHandle.Complete()
        return self.ctx.wrap(self.work.ptr, 2, dtype=np.int32).ToArray()

    @property
    def passes(self):
        """Passes of the last run that did work (the launches after them returned at once); None before the first run."""
        s = self._status()
        return None if s is None else int(s[0])

    @property
    def converged(self):
        """Whether the last run reached the fixed point within maxPasses; None before the first run."""
        s = self._status()
        return None if s is None else bool(s[1])

    def Schedule(self, requirements, dependency):
        d = requirements.data
        if not isinstance(d, GeneratorData):
            raise Exception("Unhandled stageio %s" % type(d).__name__)
        self.resolution, self.count = d.resolution, getattr(d, "count", 1)
        self.CheckRequirements(GeneratorData, requirements)
        n = self.count * self.resolution * self.resolution
        for name, m in (("rainMap", self.rainMap), ("out", self.out)):  # before any launch
            if m is not None and m.Length != n:
                raise ValueError("%s.%s holds %d floats, the payload %d" % (type(self).__name__, name, m.Length, n))
        # sized on (resolution, count) like DepressionFillStage's: the per-tile bytes depend on the number of 64 x 16 tiles
        single, batched, floats = self._ENTRIES
        need = getattr(N.lib, floats)(self.resolution, self.count)
        if self.work is None or self.work.Length != need:
            if self.work is not None and self.work.IsCreated:
                self.work.Dispose()
            self.work = self.ctx.alloc(need)
        if self.out is not None and self._plane is not None:
            self._plane.Dispose()
            self._plane = None
        if self.out is None and (self._plane is None or self._plane.Length != n):
            if self._plane is not None:
                self._plane.Dispose()
            self._plane = self.ctx.alloc(n)
        desc = self._desc(self.rainMap.ptr if self.rainMap is not None else None)
        if isinstance(d, GeneratorDataBatch):
            self.jobHandle = self.ctx.call(batched, d.data.ptr, self.drainage.ptr, self.work.ptr,
                                           C.byref(desc), d.resolution, d.count, dep=dependency)
        else:
            self.jobHandle = self.ctx.call(single, d.data.ptr, self.drainage.ptr, self.work.ptr, C.byref(desc),
                                           d.resolution, dep=dependency)

    def OnDestroy(self):
        self.DisposeArrays()


class FlowRouting(enum.IntEnum):  # new-framework: how ImplicitFluvialStage routes the drainage area
    Steepest = 0  # nz_drainage_area: all of a cell's water to its steepest neighbour
    Multiple = 1  # nz_drainage_mfd: every lower neighbour takes a slope-weighted share


class MfdDrainageStage(DrainageAreaStage):
    """Multiple-flow drainage (new-framework feature; the model is the comment block of nz_drainage_mfd in
    include/noize_hip.h): the flow accumulation of the payload's heights with every lower neighbour taking a share
    (slope / steepest slope) ^ exponent of a cell's water, normalised -- no parallel one-cell lines on hillsides, and water
    spreads on fans.  The stage is DrainageAreaStage in every other respect: the heights pass through, `drainage`, `passes`
    and `converged` describe the last payload, seaLevel, rainMap and out mean the same, a budget that runs out leaves the
    start state and converged False, and the plane is read wherever a drainage plane is.

    exponent: 1..16; 1 spreads most, larger values approach DrainageAreaStage.  maxPasses: None means
    128 + resolution // 2, twice DrainageAreaStage's: the flow graph's paths are longer than the tree's."""

    _ENTRIES = ("nz_drainage_mfd", "nz_drainage_mfd_batch", "nz_drainage_mfd_work_floats")

    def __init__(self, ctx, rain=1.0, seaLevel=DrainageAreaStage.SEA_OFF, exponent=1, maxPasses=None, rainMap=None, out=None):
        super().__init__(ctx, rain, seaLevel, maxPasses, rainMap, out)
        self.exponent = exponent

    def _desc(self, rainMap):
        budget = self.maxPasses if self.maxPasses is not None else 128 + self.resolution // 2
        return N.DrainageMfdDesc(self.rain, self.seaLevel, budget, self.exponent, rainMap)


class WatershedStage(PipelineStage):
    """Watershed (new-framework feature; the model is the comment block of nz_watershed in include/noize_hip.h): the
    steepest-descent tree of the payload's heights read upstream -- which outlet or pit every cell drains to, how far along
    the river it lies, and the tree itself.  The heights pass through untouched.  Once the stage's handle completes, `basin`
    holds the labels of the last payload (count * resolution^2 int32, the index of the outlet or pit inside the cell's own
    tile), `length` the flow-path length to it and `receivers` one code per cell (0..7 in the order W E S N SW SE NW NE, 8
    without a receiver); `passes` and `converged` are the status words of that run.  Behind DepressionFillStage every label
    lies on the border.

    seaLevel: cells at or below it are outlets like the border cells (the default, -FLT_MAX, switches it off).  cellSize:
    the length of a straight move; a diagonal one is cellSize * sqrt(2).  maxPasses: the number of pass launches; None means
    64 + resolution // 4.  A budget that runs out is no error: converged is False, the labels are the cells' own indices and
    the length is zero.  length=False: labels only, no float plane is carried.  recordReceivers: keep the receiver plane."""

    SEA_OFF = -3.4028234663852886e38  # -FLT_MAX

    def __init__(self, ctx, seaLevel=SEA_OFF, cellSize=1.0, maxPasses=None, length=True, recordReceivers=False):
        super().__init__(ctx)
        self.seaLevel = seaLevel
        self.cellSize = cellSize
        self.maxPasses = maxPasses
        self.withLength = length
        self.recordReceivers = recordReceivers
        self.resolution = 0
        self.count = 0
        self.work = None        # nz_watershed_work_floats floats; its first two int32: {passes, converged}
        self._basin = None      # the label plane: count * resolution^2 cells of 4 bytes
        self._length = None     # the length plane (length=True)
        self._receivers = None  # the receiver bytes (recordReceivers)

    def DisposeArrays(self):
        for t in (self.work, self._basin, self._length, self._receivers):
            if t is not None and t.IsCreated:
                t.Dispose()
        self.work = self._basin = self._length = self._receivers = None

    @property
    def basin(self):
        """The labels of the last run as int32, or None before the first payload and after OnDestroy."""
        if self._basin is None:
            return None
        return self.ctx.wrap(self._basin.ptr, self._basin.Length, dtype=np.int32)

    @property
    def length(self):
        """The flow-length plane(s) of the last run, or None: with length=False, before the first payload and after
        OnDestroy."""
        return self._length

    @property
    def receivers(self):
        """The receiver codes of the last run (uint8), or None: without recordReceivers, before the first payload and
        after OnDestroy."""
        return self._receivers

    def _status(self):
        if self.work is None:
            return None
        self.jobHandle.Complete()
        return self.ctx.wrap(self.work.ptr, 2, dtype=np.int32).ToArray()

    @property
    def passes(self):
        """Passes of the last run that did work (the launches after them returned at once); None before the first run."""
        s = self._status()
        return None if s is None else int(s[0])

    @property
    def converged(self):
        """Whether the last run reached the fixed point within maxPasses; None before the first run."""
        s = self._status()
        return None if s is None else bool(s[1])

    def _size(self, tile, want, n, dtype=np.float32):
        """A plane of the stage: n cells when wanted, resized with the payload, disposed of when not."""
        if tile is not None and (not want or tile.Length != n):
            tile.Dispose()
            tile = None
        if want and tile is None:
            tile = self.ctx.alloc(n, dtype=dtype)
        return tile

    def Schedule(self, requirements, dependency):
        d = requirements.data
        if not isinstance(d, GeneratorData):
            raise Exception("Unhandled stageio %s" % type(d).__name__)
        self.resolution, self.count = d.resolution, getattr(d, "count", 1)
        self.CheckRequirements(GeneratorData, requirements)
        n = self.count * self.resolution * self.resolution
        # sized on (resolution, count) like DepressionFillStage's: the per-tile bytes depend on the number of 64 x 16 tiles
        need = N.lib.nz_watershed_work_floats(self.resolution, self.count, 1 if self.withLength else 0)
        if self.work is None or self.work.Length != need:
            if self.work is not None and self.work.IsCreated:
                self.work.Dispose()
            self.work = self.ctx.alloc(need)
        self._basin = self._size(self._basin, True, n)
        self._length = self._size(self._length, bool(self.withLength), n)
        self._receivers = self._size(self._receivers, bool(self.recordReceivers), n, np.uint8)
        budget = self.maxPasses if self.maxPasses is not None else 64 + self.resolution // 4
        desc = N.WatershedDesc(self.seaLevel, self.cellSize, budget)
        planes = (self._basin.ptr, self._length.ptr if self._length is not None else None,
                  self._receivers.ptr if self._receivers is not None else None, self.work.ptr)
        if isinstance(d, GeneratorDataBatch):
            self.jobHandle = self.ctx.call("nz_watershed_batch", d.data.ptr, *planes, C.byref(desc), d.resolution, d.count,
                                           dep=dependency)
        else:
            self.jobHandle = self.ctx.call("nz_watershed", d.data.ptr, *planes, C.byref(desc), d.resolution, dep=dependency)

    def OnDestroy(self):
        self.DisposeArrays()


class StreamOrderStage(PipelineStage):
    """Stream order (new-framework feature; the model is the comment block of nz_stream_order in include/noize_hip.h): the
    channel cells of the payload's heights, their Strahler order and the unbranched reaches between heads and confluences.
    The heights pass through untouched.  Once the stage's handle completes, `order` holds one byte per cell of the last
    payload (0: no channel, 1: a head reach, +1 where two reaches of the same order meet) and `links` the cell index, inside
    the cell's own tile, of the head or confluence its reach starts at (int32, -1: no channel); `passes` and `converged` are
    the status words of that run.  Strahler streams, reaches joined across confluences that keep the order, are the
    caller's to derive from the two planes.

    seaLevel: cells at or below it are outlets like the border cells (the default, -FLT_MAX, switches it off).  drainage: a
    device plane of the payload's size the caller supplies and keeps alive, the one DrainageAreaStage(out=...) wrote; a
    cell is a channel cell when its drainage >= threshold.  Without it every cell is one and threshold is not compared.
    maxPasses: the number of pass launches; None means 64 + resolution // 4.  A budget that runs out is no error: converged
    is False, order is 1 on channel cells and every channel cell is its own link.  recordLinks: carry the link plane."""

    SEA_OFF = -3.4028234663852886e38  # -FLT_MAX

    def __init__(self, ctx, seaLevel=SEA_OFF, threshold=0.0, maxPasses=None, drainage=None, recordLinks=False):
        super().__init__(ctx)
        self.seaLevel = seaLevel
        self.threshold = threshold
        self.maxPasses = maxPasses
        self.drainage = drainage
        self.recordLinks = recordLinks
        self.resolution = 0
        self.count = 0
        self.work = None    # nz_stream_order_work_floats floats; its first two int32: {passes, converged}
        self._order = None  # the order plane: count * resolution^2 bytes
        self._links = None  # the link plane (recordLinks): count * resolution^2 cells of 4 bytes

    def DisposeArrays(self):
        for t in (self.work, self._order, self._links):
            if t is not None and t.IsCreated:
                t.Dispose()
        self.work = self._order = self._links = None

    @property
    def order(self):
        """The Strahler orders of the last run (uint8), or None before the first payload and after OnDestroy."""
        return self._order

    @property
    def links(self):
        """The links of the last run as int32, or None: without recordLinks, before the first payload and after
        OnDestroy."""
        if self._links is None:
            return None
        return self.ctx.wrap(self._links.ptr, self._links.Length, dtype=np.int32)

    def _status(self):
        if self.work is None:
            return None
        self.jobHandle.Complete()
        return self.ctx.wrap(self.work.ptr, 2, dtype=np.int32).ToArray()

    @property
    def passes(self):
        """Passes of the last run that did work (the launches after them returned at once); None before the first run."""
        s = self._status()
        return None if s is None else int(s[0])

    @property
    def converged(self):
        """Whether the last run reached the fixed point within maxPasses; None before the first run."""
        s = self._status()
        return None if s is None else bool(s[1])

    def _size(self, tile, want, n, dtype=np.float32):
        """A plane of the stage: n cells when wanted, resized with the payload, disposed of when not."""
        if tile is not None and (not want or tile.Length != n):
            tile.Dispose()
            tile = None
        if want and tile is None:
            tile = self.ctx.alloc(n, dtype=dtype)
        return tile

    def Schedule(self, requirements, dependency):
        d = requirements.data
        if not isinstance(d, GeneratorData):
            raise Exception("Unhandled stageio %s" % type(d).__name__)
        self.resolution, self.count = d.resolution, getattr(d, "count", 1)
        self.CheckRequirements(GeneratorData, requirements)
        n = self.count * self.resolution * self.resolution
        if self.drainage is not None:  # before any launch: a device tile of the payload's size, nothing else
            have = getattr(self.drainage, "Length", None)
            if not hasattr(self.drainage, "ptr") or have != n or getattr(self.drainage, "dtype", np.float32) != np.float32:
                raise ValueError("StreamOrderStage.drainage must be a device tile of %d floats, the payload's size (it holds %s)"
                                 % (n, have))
        # sized on (resolution, count) like DepressionFillStage's: the per-tile bytes depend on the number of 64 x 16 tiles
        need = N.lib.nz_stream_order_work_floats(self.resolution, self.count, 1 if self.recordLinks else 0)
        if self.work is None or self.work.Length != need:
            if self.work is not None and self.work.IsCreated:
                self.work.Dispose()
            self.work = self.ctx.alloc(need)
        self._order = self._size(self._order, True, n, np.uint8)
        self._links = self._size(self._links, bool(self.recordLinks), n)
        budget = self.maxPasses if self.maxPasses is not None else 64 + self.resolution // 4
        desc = N.StreamOrderDesc(self.seaLevel, self.threshold, budget, self.drainage.ptr if self.drainage is not None else None)
        planes = (self._order.ptr, self._links.ptr if self._links is not None else None, self.work.ptr)
        if isinstance(d, GeneratorDataBatch):
            self.jobHandle = self.ctx.call("nz_stream_order_batch", d.data.ptr, *planes, C.byref(desc), d.resolution, d.count,
                                           dep=dependency)
        else:
            self.jobHandle = self.ctx.call("nz_stream_order", d.data.ptr, *planes, C.byref(desc), d.resolution, dep=dependency)

    def OnDestroy(self):
        self.DisposeArrays()


class ImplicitFluvialStage(PipelineStage):
    """Implicit stream-power fluvial erosion (new-framework feature; the model is the comment block of nz_fluvial_implicit in
    include/noize_hip.h): FluvialErosionStage's model, k sqrt(area) slope against an uplift, taken with the implicit Euler
    step along the receiver tree -- stable for every dt, so one iteration carries a time step that the explicit stage needs
    hundreds of launches for.  Per iteration the stage computes the exact drainage area of the current heights
    (nz_drainage_area, into its own plane) and then solves the step (nz_fluvial_implicit); the solve is told to proceed by
    the drainage call's converged word on the device, nothing is read back in between.  Pits stay pits: put
    DepressionFillStage in front.  The result is in the payload's `data` when the stage's handle completes.

    seaLevel: cells at or below it are outlets like the border cells (the default, -FLT_MAX, switches it off).  rainMap /
    hardness / upliftMap: device planes of the payload's size the caller supplies and keeps alive -- rain is multiplied by
    rainMap, erodibility by 1 - hardness, uplift by upliftMap.  maxPasses: the pass launches of the drainage series and of
    the solve, each; None means 64 + resolution // 4.  A budget that runs out is no error: that iteration leaves the
    heights as they were, and `steps` stays below `iterations`.

    routing: FlowRouting.Steepest (the default) or FlowRouting.Multiple; with Multiple the drainage call of every iteration
    is nz_drainage_mfd with flowExponent (1..16), chained through the same proceed word, and its budget is
    128 + resolution // 2 when maxPasses is None.  The solve still lowers each cell along its steepest receiver: only the
    area A changes.

    After the handle completes: `drainage` is the drainage area the last iteration saw, `steps` the iterations that were
    applied, `passes` the solve passes that did work over all of them, `converged` whether steps == iterations."""

    SEA_OFF = -3.4028234663852886e38  # -FLT_MAX

    def __init__(self, ctx, iterations=1, erodibility=0.05, uplift=0.002, dt=1.0, rain=1.0, seaLevel=SEA_OFF, maxPasses=None,
                 rainMap=None, hardness=None, upliftMap=None, routing=FlowRouting.Steepest, flowExponent=1):
        super().__init__(ctx)
        self.iterations = iterations
        self.erodibility = erodibility
        self.uplift = uplift
        self.dt = dt
        self.rain = rain
        self.seaLevel = seaLevel
        self.maxPasses = maxPasses
        self.rainMap = rainMap
        self.hardness = hardness
        self.upliftMap = upliftMap
        self.routing = FlowRouting(routing)
        self.flowExponent = flowExponent
        self.resolution = 0
        self.count = 0
        self.work = None           # nz_fluvial_implicit_work_floats floats
        self.drainageWork = None   # the drainage entry's work floats; its second int32: the solve's `proceed`
        self._area = None          # the drainage plane
        self._plane = None         # the heights' second plane, for a payload without a WRITE plane
        self._tally = None         # two int32: {steps applied, passes that did work}
        self._zeros = np.zeros(2, np.int32)  # what the tally is set to before a run (kept alive: the upload reads it)

    def DisposeArrays(self):
        for t in (self.work, self.drainageWork, self._area, self._plane, self._tally):
            if t is not None and t.IsCreated:
                t.Dispose()
        self.work = self.drainageWork = self._area = self._plane = self._tally = None

    @property
    def drainage(self):
        """The drainage area the last iteration saw, or None before the first payload and after OnDestroy."""
        return self._area

    def _counts(self):
        if self._tally is None:
            return None
        self.jobHandle.Complete()
        return self._tally.ToArray()

    @property
    def steps(self):
        """Iterations of the last run that were applied; None before the first run."""
        t = self._counts()
        return None if t is None else int(t[0])

    @property
    def passes(self):
        """Solve passes of the last run that did work, over all applied iterations; None before the first run."""
        t = self._counts()
        return None if t is None else int(t[1])

    @property
    def converged(self):
        """Whether every iteration of the last run was applied; None before the first run."""
        t = self._counts()
        return None if t is None else int(t[0]) == self.iterations

    def _size(self, tile, want, n, dtype=np.float32):
        """A plane of the stage: n cells when wanted, resized with the payload, disposed of when not."""
        if tile is not None and (not want or tile.Length != n):
            tile.Dispose()
            tile = None
        if want and tile is None:
            tile = self.ctx.alloc(n, dtype=dtype)
        return tile

    def Schedule(self, requirements, dependency):
        d = requirements.data
        if not isinstance(d, GeneratorData):
            raise Exception("Unhandled stageio %s" % type(d).__name__)
        self.resolution, self.count = d.resolution, getattr(d, "count", 1)
        self.CheckRequirements(GeneratorData, requirements)
        n = self.count * self.resolution * self.resolution
        for name, m in (("rainMap", self.rainMap), ("hardness", self.hardness), ("upliftMap", self.upliftMap)):
            if m is not None and m.Length != n:  # before any launch
                raise ValueError("ImplicitFluvialStage.%s holds %d floats, the payload %d" % (name, m.Length, n))
        # sized on (resolution, count) like DrainageAreaStage's: the per-tile bytes depend on the number of 64 x 16 tiles
        self.work = self._size(self.work, True, self._solve_work_floats())
        multiple = self.routing == FlowRouting.Multiple
        if multiple:
            need = N.lib.nz_drainage_mfd_work_floats(self.resolution, self.count)
        else:
            need = N.lib.nz_drainage_area_work_floats(self.resolution, self.count)
        self.drainageWork = self._size(self.drainageWork, True, need)
        self._area = self._size(self._area, True, n)
        self._plane = self._size(self._plane, d.write is None, n)
        self._tally = self._size(self._tally, True, 2, np.int32)
        budget = self.maxPasses if self.maxPasses is not None else 64 + self.resolution // 4
        opt = lambda m: m.ptr if m is not None else None
        batch = isinstance(d, GeneratorDataBatch)
        if multiple:
            mfd_budget = self.maxPasses if self.maxPasses is not None else 128 + self.resolution // 2
            drain = N.DrainageMfdDesc(self.rain, self.seaLevel, mfd_budget, self.flowExponent, opt(self.rainMap))
            entry = "nz_drainage_mfd_batch" if batch else "nz_drainage_mfd"
        else:
            drain = N.DrainageDesc(self.rain, self.seaLevel, budget, opt(self.rainMap))
            entry = "nz_drainage_area_batch" if batch else "nz_drainage_area"
        solve = N.FluvialImplicitDesc(self.erodibility, self.uplift, self.dt, self.seaLevel, budget, opt(self.hardness),
                                      opt(self.upliftMap), self.drainageWork.ptr + 4, self._tally.ptr)
        tail = (d.resolution, d.count) if batch else (d.resolution,)
        # the heights ping-pong between the payload's plane and the WRITE plane (or the stage's own)
        cur, other = d.data, d.write if d.write is not None else self._plane
        self.jobHandle = self.ctx.call("nz_tile_upload", self._tally.ptr, self._zeros.ctypes.data, 2, dep=dependency)
        for _ in range(self.iterations):
            self.ctx.call(entry, cur.ptr, self._area.ptr,
                          self.drainageWork.ptr, C.byref(drain), *tail, handle=False)
            self.jobHandle = self._enqueue_solve(batch, cur, other, solve, tail)
            cur, other = other, cur
        if d.write is not None:
            d.data, d.write = cur, other  # the pair as the run left it: `data` holds the result
        elif cur is not d.data:           # an odd count ended in the stage's plane
            self.jobHandle = self.ctx.call("nz_flush_write_slice", d.data.ptr, cur.ptr, n)

    # the hook of a stage that derives from this one (SedimentFluvialStage): the size of `work`, and the solve of one iteration
    def _solve_work_floats(self):
        return N.lib.nz_fluvial_implicit_work_floats(self.resolution, self.count)

    def _enqueue_solve(self, batch, cur, other, solve, tail):
        """Enqueue the solve of one iteration, heights `cur` -> `other`, with the FluvialImplicitDesc of the run."""
        return self.ctx.call("nz_fluvial_implicit_batch" if batch else "nz_fluvial_implicit", cur.ptr,
                             self._area.ptr, other.ptr, self.work.ptr, C.byref(solve), *tail)

    def OnDestroy(self):
        self.DisposeArrays()


class MfdFluvialStage(PipelineStage):
    """Multiple-flow implicit stream-power erosion (new-framework feature; the model is the comment block of
    nz_fluvial_implicit_mfd in include/noize_hip.h): ImplicitFluvialStage's step taken along EVERY lower neighbour of a
    cell, with the weights of MfdDrainageStage -- the water is spread over a fan and the fan is what erodes, where
    ImplicitFluvialStage(routing=FlowRouting.Multiple) cuts along the one steepest receiver.  Per iteration the stage
    computes the multiple-flow drainage of the current heights (nz_drainage_mfd, into its own plane) and then solves the
    step (nz_fluvial_implicit_mfd), both with the same `exponent` (1..16); the solve is told to proceed by the drainage
    call's converged word on the device, nothing is read back in between.  Pits stay pits: put DepressionFillStage in
    front.  The heights ping-pong between the payload's plane and its WRITE plane (or a plane of the stage's); the result
    is in the payload's `data` when the stage's handle completes.

    seaLevel: cells at or below it are outlets like the border cells (the default, -FLT_MAX, switches it off).  rainMap /
    hardness / upliftMap: device planes of the payload's size the caller supplies and keeps alive -- rain is multiplied by
    rainMap, erodibility by 1 - hardness, uplift by upliftMap.  maxPasses: the pass launches of the drainage
    series and of the solve, each; None means 128 + resolution // 2.  A budget that runs out is no error: that iteration
    leaves the heights as they were, and `steps` stays below `iterations`.

    After the handle completes: `drainage` is the drainage area the last iteration saw, `steps` the iterations that were
    applied, `passes` the solve passes that did work over all of them, `converged` whether steps == iterations."""

    SEA_OFF = -3.4028234663852886e38  # -FLT_MAX

    def __init__(self, ctx, iterations=1, erodibility=0.05, uplift=0.002, dt=1.0, rain=1.0, seaLevel=SEA_OFF, exponent=1,
                 maxPasses=None, rainMap=None, hardness=None, upliftMap=None):
        super().__init__(ctx)
        self.iterations = iterations
        self.erodibility = erodibility
        self.uplift = uplift
        self.dt = dt
        self.rain = rain
        self.seaLevel = seaLevel
        self.exponent = exponent
        self.maxPasses = maxPasses
        self.rainMap = rainMap
        self.hardness = hardness
        self.upliftMap = upliftMap
        self.resolution = 0
        self.count = 0
        self.work = None           # nz_fluvial_implicit_mfd_work_floats floats
        self.drainageWork = None   # nz_drainage_mfd's work floats; its second int32: the solve's `proceed`
        self._area = None          # the drainage plane
        self._plane = None         # the heights' second plane, for a payload without a WRITE plane
        self._tally = None         # two int32: {steps applied, passes that did work}
        self._zeros = np.zeros(2, np.int32)  # what the tally is set to before a run (kept alive: the upload reads it)

    def DisposeArrays(self):
        for t in (self.work, self.drainageWork, self._area, self._plane, self._tally):
            if t is not None and t.IsCreated:
                t.Dispose()
        self.work = self.drainageWork = self._area = self._plane = self._tally = None

    @property
    def drainage(self):
        """The drainage area the last iteration saw, or None before the first payload and after OnDestroy."""
        return self._area

    def _counts(self):
        if self._tally is None:
            return None
        self.jobHandle.Complete()
        return self._tally.ToArray()

    @property
    def steps(self):
        """Iterations of the last run that were applied; None before the first run."""
        t = self._counts()
        return None if t is None else int(t[0])

    @property
    def passes(self):
        """Solve passes of the last run that did work, over all applied iterations; None before the first run."""
        t = self._counts()
        return None if t is None else int(t[1])

    @property
    def converged(self):
        """Whether every iteration of the last run was applied; None before the first run."""
        t = self._counts()
        return None if t is None else int(t[0]) == self.iterations

    def _size(self, tile, want, n, dtype=np.float32):
        """A plane of the stage: n cells when wanted, resized with the payload, disposed of when not."""
        if tile is not None and (not want or tile.Length != n):
            tile.Dispose()
            tile = None
        if want and tile is None:
            tile = self.ctx.alloc(n, dtype=dtype)
        return tile


    def Schedule(self, requirements, dependency):
        d = requirements.data
        if not isinstance(d, GeneratorData):
            raise Exception("Unhandled stageio %s" % type(d).__name__)
        self.resolution, self.count = d.resolution, getattr(d, "count", 1)
        self.CheckRequirements(GeneratorData, requirements)
        n = self.count * self.resolution * self.resolution
        for name, m in (("rainMap", self.rainMap), ("hardness", self.hardness), ("upliftMap", self.upliftMap)):
            if m is not None and m.Length != n:  # before any launch
                raise ValueError("MfdFluvialStage.%s holds %d floats, the payload %d" % (name, m.Length, n))
        self.work = self._size(self.work, True, N.lib.nz_fluvial_implicit_mfd_work_floats(self.resolution, self.count))
        self.drainageWork = self._size(self.drainageWork, True, N.lib.nz_drainage_mfd_work_floats(self.resolution, self.count))
        self._area = self._size(self._area, True, n)
        self._plane = self._size(self._plane, d.write is None, n)
        self._tally = self._size(self._tally, True, 2, np.int32)
        budget = self.maxPasses if self.maxPasses is not None else 128 + self.resolution // 2
        opt = lambda m: m.ptr if m is not None else None
        batch = isinstance(d, GeneratorDataBatch)
        drain = N.DrainageMfdDesc(self.rain, self.seaLevel, budget, self.exponent, opt(self.rainMap))
        # the solve's `proceed`: the drainage call's converged word, the second int32 of its work planes
        solve = N.FluvialImplicitMfdDesc(self.erodibility, self.uplift, self.dt, self.seaLevel, budget, self.exponent,
                                         opt(self.hardness), opt(self.upliftMap), self.drainageWork.ptr + 4, self._tally.ptr)
        tail = (d.resolution, d.count) if batch else (d.resolution,)
        # the heights ping-pong between the payload's plane and the WRITE plane (or the stage's own)
        cur, other = d.data, d.write if d.write is not None else self._plane
        self.jobHandle = self.ctx.call("nz_tile_upload", self._tally.ptr, self._zeros.ctypes.data, 2, dep=dependency)
        for _ in range(self.iterations):
            self.ctx.call("nz_drainage_mfd_batch" if batch else "nz_drainage_mfd", cur.ptr, self._area.ptr,
                          self.drainageWork.ptr, C.byref(drain), *tail, handle=False)
            self.jobHandle = self.ctx.call("nz_fluvial_implicit_mfd_batch" if batch else "nz_fluvial_implicit_mfd", cur.ptr,
                                           self._area.ptr, other.ptr, self.work.ptr, C.byref(solve), *tail)
            cur, other = other, cur
        if d.write is not None:
            d.data, d.write = cur, other  # the pair as the run left it: `data` holds the result
        elif cur is not d.data:           # an odd count ended in the stage's plane
            self.jobHandle = self.ctx.call("nz_flush_write_slice", d.data.ptr, cur.ptr, n)

    def OnDestroy(self):
        self.DisposeArrays()


class HillslopeDiffusionStage(PipelineStage):
    """Linear hillslope diffusion, dh/dt = diffusivity * laplace(h), as implicit steps of any size (new-framework feature;
    the model is the comment block of nz_hillslope_diffusion in include/noize_hip.h): backward Euler split by direction, two
    tridiagonal line solves per step, stable and free of oscillation for every dt, the border cells held.  It is the term
    that rounds the knife-edge ridges and one-cell gullies ImplicitFluvialStage leaves; the evolution loop is
    [DepressionFillStage, ImplicitFluvialStage(dt=T), HillslopeDiffusionStage(dt=T)], repeated.  A direct solve: no pass
    budget, no verdict, nothing read back.  The stage works in place on the payload's `data` (GeneratorData and
    GeneratorDataBatch) and owns and resizes its `work`, the two coefficient tables.

    The defaults -- diffusivity 0.01, dt 1, iterations 1 -- are a choice, not pinned by any picture: r = diffusivity * dt is
    what the result depends on, and `iterations` steps of dt are not one step of iterations * dt."""

    def __init__(self, ctx, diffusivity=0.01, dt=1.0, iterations=1):
        super().__init__(ctx)
        self.diffusivity = diffusivity
        self.dt = dt
        self.iterations = iterations
        self.resolution = 0
        self.count = 0
        self.work = None  # nz_hillslope_diffusion_work_floats floats

    def DisposeArrays(self):
        if self.work is not None and self.work.IsCreated:
            self.work.Dispose()
        self.work = None

    def Schedule(self, requirements, dependency):
        d = requirements.data
        if not isinstance(d, GeneratorData):
            raise Exception("Unhandled stageio %s" % type(d).__name__)
        self.resolution, self.count = d.resolution, getattr(d, "count", 1)
        self.CheckRequirements(GeneratorData, requirements)
        need = N.lib.nz_hillslope_diffusion_work_floats(self.resolution, self.count)
        if self.work is not None and self.work.Length != need:
            self.DisposeArrays()
        if self.work is None:
            self.work = self.ctx.alloc(need)
        desc = N.HillslopeDesc(self.diffusivity, self.dt, self.iterations)
        batch = isinstance(d, GeneratorDataBatch)
        tail = (d.resolution, d.count) if batch else (d.resolution,)
        self.jobHandle = self.ctx.call("nz_hillslope_diffusion_batch" if batch else "nz_hillslope_diffusion", d.data.ptr,
                                       d.data.ptr, self.work.ptr, C.byref(desc), *tail, dep=dependency)

    def OnDestroy(self):
        self.DisposeArrays()


class SedimentFluvialStage(ImplicitFluvialStage):
    """Implicit stream-power erosion WITH sediment deposition (new-framework feature; the model is the comment block of
    nz_fluvial_sediment in include/noize_hip.h): ImplicitFluvialStage whose solve carries the xi-q deposition term, so
    valleys aggrade as well as cut.  Everything but the solve call is inherited: per iteration the drainage call (either
    routing), the proceed word, the plane ping-pong, steps / passes / converged and the resize logic.

    deposition: G >= 0, dimensionless; 0 is ImplicitFluvialStage bit for bit.  sedimentIterations: the Gauss-Seidel
    iterations K of every solve; the iteration contracts for G up to about 1, slower as G * dt grows -- read `residual`.
    recordFlux: keep the sediment-flux plane Q of the last applied iteration in `flux`.  maxPasses is the budget of each of
    the 2K + 1 series of a solve, and `passes` counts them all.

    After the handle completes: `residual` is max |hK - h(K-1)| of the last iteration that ran (0.0 when it was not
    applied), `flux` the stage's own flux plane (None without recordFlux)."""

    def __init__(self, ctx, iterations=1, erodibility=0.05, uplift=0.002, dt=1.0, rain=1.0, seaLevel=ImplicitFluvialStage.SEA_OFF,
                 maxPasses=None, rainMap=None, hardness=None, upliftMap=None, routing=FlowRouting.Steepest, flowExponent=1,
                 deposition=0.5, sedimentIterations=4, recordFlux=False):
        super().__init__(ctx, iterations, erodibility, uplift, dt, rain, seaLevel, maxPasses, rainMap, hardness, upliftMap,
                         routing, flowExponent)
        self.deposition = deposition
        self.sedimentIterations = sedimentIterations
        self.recordFlux = recordFlux
        self._flux = None  # the flux plane, with recordFlux

    def DisposeArrays(self):
        if self._flux is not None and self._flux.IsCreated:
            self._flux.Dispose()
        self._flux = None
        super().DisposeArrays()

    @property
    def flux(self):
        """The sediment flux Q of the last applied iteration; None without recordFlux, before the first payload and after
        OnDestroy."""
        return self._flux

    @property
    def residual(self):
        """max |hK - h(K-1)| of the last iteration that ran; None before the first run."""
        if self._tally is None:
            return None
        self.jobHandle.Complete()
        return float(self.ctx.wrap(self.work.ptr, 3, dtype=np.int32).ToArray().view(np.float32)[2])

    def _solve_work_floats(self):
        return N.lib.nz_fluvial_sediment_work_floats(self.resolution, self.count)

    def _enqueue_solve(self, batch, cur, other, solve, tail):
        self._flux = self._size(self._flux, bool(self.recordFlux), self.count * self.resolution * self.resolution)
        desc = N.FluvialSedimentDesc(*[getattr(solve, f[0]) for f in N.FluvialImplicitDesc._fields_], self.deposition,
                                     self.sedimentIterations, self._flux.ptr if self._flux is not None else None)
        return self.ctx.call("nz_fluvial_sediment_batch" if batch else "nz_fluvial_sediment", cur.ptr, self._area.ptr,
                             other.ptr, self.work.ptr, C.byref(desc), *tail)


class MeshTileStage(PipelineStage):  # Mesh/Stage/MeshTileStage.cs:28-61
    def __init__(self, ctx, meshType=MeshType.SquareGridHeightMap):
        super().__init__(ctx)
        self.meshType = meshType
        self.currentMesh = None

    def Schedule(self, requirements, dependency):
        d = requirements.data  # (MeshStageData) cast
        if not isinstance(d, MeshStageData):
            raise Exception("Unhandled stageio %s" % type(d).__name__)
        self.currentMesh = d.mesh if d.mesh is not None else MeshBuffers()
        d.mesh = self.currentMesh
        m = self.currentMesh
        count = getattr(d, "count", 1)
        nv, ni = N.lib.nz_mesh_vertex_count(d.resolution) * count, N.lib.nz_mesh_index_count(d.resolution) * count
        if m.vertexCount != nv or m.vertices is None:  # Mesh.AllocateWritableMeshData(1)
            m.vertices = self.ctx.alloc(nv * 12)
            m.indices = self.ctx.alloc(ni, dtype=np.uint32)
            m.vertexCount, m.indexCount = nv, ni
        if count > 1:
            self.jobHandle = self.ctx.call("nz_heightmap_mesh_batch", int(self.meshType), m.vertices.ptr, m.indices.ptr,
                                           d.resolution, d.inputResolution, d.marginPix, d.tileHeight, d.tileSize,
                                           d.data.ptr, count, dep=dependency)
            return
        self.jobHandle = self.ctx.call("nz_heightmap_mesh", int(self.meshType), m.vertices.ptr, m.indices.ptr,
                                       d.resolution, d.inputResolution, d.marginPix, d.tileHeight, d.tileSize,
                                       d.data.ptr, dep=dependency)


# ---- BasePipeline -------------------------------------------------------------------------------
class BasePipeline:  # Pipeline/Executable/Pipeline.cs:19-287
    def __init__(self, stages, alias="Unnamed Pipeline", contextManager=None):
        self.alias = alias
        self.contextManager = contextManager  # PipelineStateManager handed to every work item (:76-104)
        self.queue = collections.deque()  # ConcurrentQueue: deque.append is thread-safe
        self.dependencyHell = []
        self.activeItem = None
        self.pipelineHandle = JobHandle()
        self.pipelineBeingScheduled = False
        self.pipelineRunning = False
        self.stage_instances = list(stages) if stages is not None else None
        self.Setup()
        self.pipeLineReady = True

    def Setup(self):  # :130-152
        if not self.stage_instances:
            return
        previous = None
        for stage in self.stage_instances:
            if previous is not None:
                previous.OnStageScheduledAction.append(stage.ReceiveHandledInput)
            previous = stage
        self.stage_instances[-1].OnStageScheduledAction.append(self.OnPipelineFullyScheduled)

    def Enqueue(self, input, scheduleAction=None, completeAction=None, dependency=None):  # :76-90
        self.queue.append(PipelineWorkItem(input, completeAction, scheduleAction, dependency, self.contextManager))

    def Schedule(self, input=None, scheduleAction=None, completeAction=None, dependency=None):  # :91-120
        if isinstance(input, PipelineWorkItem):
            self.activeItem = input
        elif input is not None:
            self.activeItem = PipelineWorkItem(input, completeAction, scheduleAction, dependency, self.contextManager)
        if not self.stage_instances:
            raise Exception("No stages in pipeline")
        self.pipelineBeingScheduled = True
        self.stage_instances[0].ReceiveHandledInput(self.activeItem, self.activeItem.dependency)

    def OnPipelineFullyScheduled(self, res, handle):  # :122-128
        self.pipelineHandle = handle
        self.pipelineRunning = True
        self.pipelineBeingScheduled = False
        if self.activeItem.scheduledAction:
            self.activeItem.scheduledAction(res.data, handle)

    def WorkIsSchedulable(self, item):  # :256-265
        ready = True
        for stage in self.stage_instances:
            ready = stage.IsSchedulable(item) and ready
        return ready

    def GetNextJob(self):  # :183-214
        for i, job in enumerate(list(self.dependencyHell)):
            if self.WorkIsSchedulable(job):
                self.dependencyHell.remove(job)
                return job
        while self.queue:
            wi = self.queue.popleft()
            if self.WorkIsSchedulable(wi):
                return wi
            self.dependencyHell.append(wi)
        return None

    def Update(self):  # :154-158,224-230
        if not self.pipelineRunning and not self.pipelineBeingScheduled:
            job = self.GetNextJob()
            if job is not None:
                self.Schedule(job)

    def _retry_is_local(self):
        """Nobody outside this pipeline has been handed a handle of the pass that is running: the work item carries no
        scheduledAction, and no stage has a scheduled-action hook beyond the hand-over to the next stage (a joint, a
        downstream pipeline's OnScheduledUpstream).  Work scheduled on such a handle has consumed the failed pass's planes
        and cannot be recalled from here."""
        own = {s.ReceiveHandledInput for s in self.stage_instances} | {self.OnPipelineFullyScheduled}
        return self.activeItem.scheduledAction is None and all(a in own for s in self.stage_instances
                                                               for a in s.OnStageScheduledAction)

    def _complete(self):
        """pipelineHandle.Complete().  NZ_ERR_RETRY -- a chained kernel-filter launch timed out, the planes computed since
        are invalid and the context has switched to separate launches -- is answered once by running the work item again,
        when (a) the pipeline regenerates its tile from scratch (its first stage is the NoiseStage) and (b) the failed pass
        is this pipeline's own business (_retry_is_local).  The failed pass is wound up first (the stages' OnStageComplete,
        as after any pass), then the item is scheduled as a retry: its dependency was satisfied by the first pass and is
        not applied again.  Any other pipeline's input is gone with the stage that failed, or its handles are in other
        hands: the error goes to the caller."""
        try:
            self.pipelineHandle.Complete()
        except N.NoizeError as e:
            if e.status != N.NZ_ERR_RETRY or not isinstance(self.stage_instances[0], NoiseStage) or not self._retry_is_local():
                raise
            self.CleanUp()
            self.pipelineRunning = False
            item = self.activeItem
            item.dependency, item.retries = JobHandle(), getattr(item, "retries", 0) + 1
            self.Schedule(item)
            self.pipelineHandle.Complete()  # (a second failure is the caller's)

    def LateUpdate(self):  # :160-181
        if self.pipelineRunning and self.pipelineHandle.IsCompleted:
            self._complete()
            self.CleanUp()
            if self.activeItem.completeAction:
                self.activeItem.completeAction(self.activeItem.data)
            self.pipelineRunning = False
            return True
        return False

    def CleanUp(self):  # :232-242
        for stage in self.stage_instances:
            stage.OnStageComplete()

    def RunToCompletion(self):
        """Drive Update/LateUpdate (Unity's frame loop) until the queue is drained."""
        while self.queue or self.dependencyHell or self.pipelineRunning:
            self.Update()
            if self.pipelineRunning:
                self._complete()
                self.LateUpdate()

    def GetDependencies(self):  # :63-65
        return [self]

    def Destroy(self):  # :244-254,267-274
        for stage in self.stage_instances:
            stage.OnDestroy()


class Upstream(enum.IntEnum):  # Pipeline/Executable/ReducePipeline.cs:27-30
    LEFT = 0
    RIGHT = 1


class PipelineJoint:  # ReducePipeline.cs:18-25
    def __init__(self, stages, action):
        self.stages = stages
        self.status = {Upstream.LEFT: False, Upstream.RIGHT: False}
        self.action = action

    @property
    def ready(self):
        return self.status[Upstream.LEFT] and self.status[Upstream.RIGHT]


class ReducePipeline(BasePipeline):  # Pipeline/Executable/ReducePipeline.cs:31-166
    """Takes one work item, requests the same tile from both upstream pipelines (the right one into a
    plane this pipeline owns) and, once both have completed, runs its own stages on a ReduceData of the
    two planes.  `ctx` allocates the right-hand plane (the reference's Persistent NativeArray)."""

    def __init__(self, ctx, stages, upstreamPipelineLeft, upstreamPipelineRight, alias="Unnamed Pipeline",
                 contextManager=None, deviceJoin=False):
        super().__init__(stages, alias, contextManager)
        self.ctx = ctx
        # deviceJoin (new-framework): the upstream pipelines may run on other contexts (HIP streams).  Instead of
        # waiting on the host for both to COMPLETE (the reference polls JobHandle.IsCompleted, :123-149), this
        # pipeline's stages are scheduled as soon as both upstreams are SCHEDULED, with
        # JobHandle.CombineDependencies(left, right) as their dependency: the join happens on the device
        # (hipStreamWaitEvent), the host never blocks between the three pipelines.
        self.deviceJoin = deviceJoin
        self._scheduled = {}
        self.upstreamPipelineLeft = upstreamPipelineLeft
        self.upstreamPipelineRight = upstreamPipelineRight
        self.upstreamsRunning = False
        self.currentWorkItem = None
        self.currentDataLength = 0
        self.rightData = None

    def GetDependencies(self):  # :52-62
        return ([self.upstreamPipelineLeft, self.upstreamPipelineRight, self] +
                self.upstreamPipelineLeft.GetDependencies() + self.upstreamPipelineRight.GetDependencies())

    def Update(self):  # OnUpdate :64-80
        if not self.pipelineRunning and not self.pipelineBeingScheduled and not self.upstreamsRunning:
            if self.queue:
                wi = self.queue.popleft()
                self.upstreamsRunning = True
                self.ScheduleUpstreams(wi)

    def ScheduleUpstreams(self, wi):  # :82-121
        leftData = wi.data
        if not isinstance(leftData, GeneratorData):
            raise Exception("Unhandled stageio %s" % type(leftData).__name__)
        if leftData.data.Length != self.currentDataLength:
            self.currentDataLength = leftData.data.Length
            if self.rightData is not None and self.rightData.IsCreated:
                self.rightData.Dispose()
            self.rightData = self.ctx.alloc(self.currentDataLength)
        if self.rightData is None or not self.rightData.IsCreated:
            self.rightData = self.ctx.alloc(self.currentDataLength)
        self.currentWorkItem = PipelineJoint(
            {Upstream.LEFT: leftData,
             Upstream.RIGHT: GeneratorData(leftData.uuid, self.rightData, leftData.resolution, leftData.xpos,
                                           leftData.zpos)},
            wi.completeAction)
        if self.deviceJoin:
            self._scheduled = {}
            self.upstreamPipelineLeft.Enqueue(self.currentWorkItem.stages[Upstream.LEFT],
                                              scheduleAction=lambda res, h: self.OnScheduledUpstream(res, h, Upstream.LEFT))
            self.upstreamPipelineRight.Enqueue(self.currentWorkItem.stages[Upstream.RIGHT],
                                               scheduleAction=lambda res, h: self.OnScheduledUpstream(res, h, Upstream.RIGHT))
            return
        self.upstreamPipelineLeft.Enqueue(self.currentWorkItem.stages[Upstream.LEFT], completeAction=self.OnCompleteLeft)
        self.upstreamPipelineRight.Enqueue(self.currentWorkItem.stages[Upstream.RIGHT],
                                           completeAction=self.OnCompleteRight)

    def OnScheduledUpstream(self, res, handle, side):
        """deviceJoin: an upstream has enqueued all its work; `handle` is its pipelineHandle."""
        self._scheduled[side] = handle
        self.currentWorkItem.status[side] = True
        self.currentWorkItem.stages[side] = res
        if self.currentWorkItem.ready:
            self.upstreamsRunning = False
            j = self.currentWorkItem
            dep = JobHandle.CombineDependencies(self.stage_instances[0].ctx, self._scheduled[Upstream.LEFT],
                                                self._scheduled[Upstream.RIGHT])
            self.Schedule(ReduceData(res.uuid, j.stages[Upstream.LEFT].data, j.stages[Upstream.RIGHT].data,
                                     res.resolution, res.xpos, res.zpos), completeAction=j.action, dependency=dep)

    def OnCompleteUpstream(self, res, side):  # :123-149
        self.currentWorkItem.status[side] = True
        self.currentWorkItem.stages[side] = res
        if self.currentWorkItem.ready:
            self.upstreamsRunning = False
            j = self.currentWorkItem
            self.Schedule(ReduceData(res.uuid, j.stages[Upstream.LEFT].data, j.stages[Upstream.RIGHT].data,
                                     res.resolution, res.xpos, res.zpos), completeAction=j.action)

    def OnCompleteLeft(self, res):
        self.OnCompleteUpstream(res, Upstream.LEFT)

    def OnCompleteRight(self, res):
        self.OnCompleteUpstream(res, Upstream.RIGHT)

    def RunToCompletion(self):
        """Unity's frame loop over this pipeline and everything upstream of it."""
        pipes = []
        for pl in self.GetDependencies():
            if pl not in pipes:
                pipes.append(pl)
        busy = True
        while busy:
            for pl in pipes:
                pl.Update()
            for pl in pipes:
                if pl.pipelineRunning:
                    pl.pipelineHandle.Complete()
                    pl.LateUpdate()
            busy = any(pl.queue or pl.dependencyHell or pl.pipelineRunning or pl.pipelineBeingScheduled or
                       getattr(pl, "upstreamsRunning", False) for pl in pipes)

    def Destroy(self):  # :157-163
        if self.rightData is not None and self.rightData.IsCreated:
            self.rightData.Dispose()
        super().Destroy()
