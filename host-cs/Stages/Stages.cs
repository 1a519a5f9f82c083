// Stages.cs -- the stage classes of the hot path with the reference's fields and Schedule bodies; where the reference
// calls a static Burst-job delegate, these call the C ABI (one extern "C" entry per delegate, include/noize_hip.h).
//   NoiseStage            Noise/NoiseStage.cs:13-61
//   ShapedNoiseStage      new-framework: NoiseStage with an octave shape (billow, ridged multifractal)
//   WarpedNoiseStage      new-framework: ShapedNoiseStage at domain-warped coordinates
//   KernelFilterStage     Filter/KernelFilterStage.cs:13-51
//   StageGaussianBlur     Filter/Kernel/Blur/StageGaussianBlur.cs:14-53
//   StageSmoothBlur       Filter/Kernel/Blur/StageSmoothBlur.cs:14-52
//   ErosionStage          ErosionKernelJob (Filter/Kernel/KernelJob.cs:317-350) in KernelFilterStage's shape
//   FlowMapStage          Geologic/Stage/FlowMapStage.cs:16-220
//   MeshTileStage         Mesh/Stage/MeshTileStage.cs:28-61
//   ConstantStage / ReduceStage / CurveStage   Filter/ConstantStage.cs, Filter/Reduce/ReduceStage.cs, Filter/Curve/CurveStage.cs
//   CropStage             Filter/Sample/CropStage.cs:11-19
//   StageThermalErosion   Filter/Kernel/Blur/StageThermalErosion.cs:12-29
// Source only (no .NET toolchain in the build image).
using System;

namespace xshazwar.noize.hip {

    public enum FractalNoise { Sin, Perlin, PeriodicPerlin, Simplex, RotatedSimplex, Cellular, DomainRotatedPerlin, DomainRotatedSimplex }  // NoiseStage.cs:15-24
    public enum FractalShape { Fbm, Billow, Ridged }                                                                                     // enum nz_fractal_shape
    public enum KernelFilterType { Gauss9_S1, Gauss7_S1, Gauss5_S1, Gauss3_S1, Gauss9_S2, Gauss7_S2, Gauss5_S2, Gauss3_S2, Smooth3,
                                   Sobel3Horizontal, Sobel3Vertical, Sobel3_2D, Prewitt3Horizontal, Prewitt3Vertical }                  // KernelJob.cs:79-94
    public enum GaussSigma { s0d50, s1d00, s1d50, s2d00, s2d50, s3d00, s3d50, s4d00, s4d50, s5d00, s5d50, s6d00, s6d50, s7d00, s7d50, s8d00 } // BlurKernels.cs:8-25
    public enum MeshType { SquareGridHeightMap, OvershootSquareGridHeightMap }                                                           // MeshTileStage.cs:23-26
    public enum ConstantOperationType { MULTIPLY, BINARIZE }                                                                             // ConstantStage.cs:15-18
    public enum ReductionType { SUBTRACT, MULTIPLY, ROOTSUMSQUARES, MAX, MIN }                                                           // ReduceStage.cs:12-18

    public static class BlurHelper {             // BlurKernels.cs:27-37
        public const int max_width = 25;
        public static int limitWidth(int width) {
            if (width % 2 == 0) width += 1;
            width = Math.Min(width, max_width);
            return Math.Max(3, width);
        }
    }

    public abstract class TmpStage : PipelineStage {   // the `tmp` NativeArray the filter stages own (KernelFilterStage.cs:22-29)
        protected DeviceTile tmp;
        protected static int BatchCount(GeneratorData d) => d is GeneratorDataBatch b ? b.count : 1;
        protected TmpStage(GpuContext ctx) : base(ctx) {}
        public override void ResizeNativeContainers(int size) { tmp?.Dispose(); tmp = ctx.Alloc(size); }
        public override void OnDestroy() { tmp?.Dispose(); tmp = null; }
    }

    public class NoiseStage : PipelineStage {
        public FractalNoise noiseType = FractalNoise.Sin;
        public float hurst = 0f, startingAmplitude = 1f, stepdown = 2f, detuneRate = 0f;
        public int octaves = 1, noiseSize = 1000;
        public NoiseStage(GpuContext ctx) : base(ctx) {}
        public override void Schedule(PipelineWorkItem requirements, GpuJobHandle dependency) {     // :55-60
            CheckRequirements<GeneratorData>(requirements);
            GeneratorData d = (GeneratorData) requirements.data;
            if (d is GeneratorDataBatch b) {      // `count` tiles, one launch
                Native.Check(Native.nz_fractal_batch(ctx.Handle, (int) noiseType, b.data.Ptr, b.resolution, b.count, b.positions.Ptr, hurst,
                                                     startingAmplitude, stepdown, detuneRate, octaves, noiseSize, dependency.id, out ulong hb), "nz_fractal_batch");
                jobHandle = Done(hb);
                return;
            }
            // jobs[(int) noiseType](d.data, d.resolution, hurst, startingAmplitude, stepdown, detuneRate, octaves, d.xpos, d.zpos, noiseSize, dependency)
            Native.Check(Native.nz_fractal(ctx.Handle, (int) noiseType, d.data.Ptr, d.resolution, hurst, startingAmplitude, stepdown,
                                           detuneRate, octaves, d.xpos, d.zpos, noiseSize, dependency.id, out ulong h), "nz_fractal");
            jobHandle = Done(h);
        }
    }

    // NoiseStage with an octave shape; Fbm gives the bits of NoiseStage.  BasePipeline.StockListParams compares the exact type,
    // so a shaped stage never runs there as plain fBm.
    public class ShapedNoiseStage : NoiseStage {
        public FractalShape shape = FractalShape.Ridged;
        public float ridgeOffset = 1f, ridgeGain = 2f;
        public ShapedNoiseStage(GpuContext ctx) : base(ctx) {}
        public override void Schedule(PipelineWorkItem requirements, GpuJobHandle dependency) {
            CheckRequirements<GeneratorData>(requirements);
            GeneratorData d = (GeneratorData) requirements.data;
            if (d is GeneratorDataBatch b) {
                Native.Check(Native.nz_fractal_shaped_batch(ctx.Handle, (int) noiseType, b.data.Ptr, b.resolution, b.count, b.positions.Ptr,
                                                            hurst, startingAmplitude, stepdown, detuneRate, octaves, noiseSize, (int) shape,
                                                            ridgeOffset, ridgeGain, dependency.id, out ulong hb), "nz_fractal_shaped_batch");
                jobHandle = Done(hb);
                return;
            }
            Native.Check(Native.nz_fractal_shaped(ctx.Handle, (int) noiseType, d.data.Ptr, d.resolution, hurst, startingAmplitude, stepdown,
                                                  detuneRate, octaves, d.xpos, d.zpos, noiseSize, (int) shape, ridgeOffset, ridgeGain,
                                                  dependency.id, out ulong h), "nz_fractal_shaped");
            jobHandle = Done(h);
        }
    }

    // ShapedNoiseStage read at domain-warped coordinates: each cell moves by (2q - 1) * warpStrength cells, q a plain fBm of the
    // same basis over warpOctaves octaves at warpScale times the noise's frequency.  warpStrength 0 or warpOctaves 0 gives the
    // bits of ShapedNoiseStage.
    public class WarpedNoiseStage : ShapedNoiseStage {
        public float warpStrength = 0f, warpScale = 1f;
        public int warpOctaves = 4;
        public WarpedNoiseStage(GpuContext ctx) : base(ctx) { shape = FractalShape.Fbm; }
        public override void Schedule(PipelineWorkItem requirements, GpuJobHandle dependency) {
            CheckRequirements<GeneratorData>(requirements);
            GeneratorData d = (GeneratorData) requirements.data;
            if (d is GeneratorDataBatch b) {
                Native.Check(Native.nz_fractal_warped_batch(ctx.Handle, (int) noiseType, b.data.Ptr, b.resolution, b.count, b.positions.Ptr,
                                                            hurst, startingAmplitude, stepdown, detuneRate, octaves, noiseSize, (int) shape,
                                                            ridgeOffset, ridgeGain, warpStrength, warpScale, warpOctaves, dependency.id,
                                                            out ulong hb), "nz_fractal_warped_batch");
                jobHandle = Done(hb);
                return;
            }
            Native.Check(Native.nz_fractal_warped(ctx.Handle, (int) noiseType, d.data.Ptr, d.resolution, hurst, startingAmplitude, stepdown,
                                                  detuneRate, octaves, d.xpos, d.zpos, noiseSize, (int) shape, ridgeOffset, ridgeGain,
                                                  warpStrength, warpScale, warpOctaves, dependency.id, out ulong h), "nz_fractal_warped");
            jobHandle = Done(h);
        }
    }

    public class KernelFilterStage : TmpStage {
        public KernelFilterType filter = KernelFilterType.Gauss9_S1;
        public int iterations = 1;
        public KernelFilterStage(GpuContext ctx) : base(ctx) {}
        public override void Schedule(PipelineWorkItem requirements, GpuJobHandle dependency) {     // :31-43
            CheckRequirements<GeneratorData>(requirements);
            GeneratorData d = (GeneratorData) requirements.data;
            ulong h;
            if (d.write != null && filter != KernelFilterType.Sobel3_2D) {
                NzRwTile t = new NzRwTile { read = d.data.Ptr, write = d.write.Ptr, resolution = d.resolution, count = BatchCount(d) };
                Native.Check(Native.nz_kernel_filter_stage_rw(ctx.Handle, ref t, (int) filter, iterations, dependency.id, out h), "nz_kernel_filter_stage_rw");
                Adopt(d, t);
            } else if (d is GeneratorDataBatch b) {
                Native.Check(Native.nz_kernel_filter_stage_batch(ctx.Handle, b.data.Ptr, tmp.Ptr, (int) filter, iterations, b.resolution, b.count, dependency.id, out h), "nz_kernel_filter_stage_batch");
            } else {
                // the reference chains `iterations` SeparableKernelFilter.Schedule calls (:35-41); the library fuses the chain
                Native.Check(Native.nz_kernel_filter_stage(ctx.Handle, d.data.Ptr, tmp.Ptr, (int) filter, iterations, d.resolution, dependency.id, out h), "nz_kernel_filter_stage");
            }
            jobHandle = Done(h);
        }
    }

    public class StageGaussianBlur : TmpStage {
        public int iterations = 1, width = 3;
        public GaussSigma sigma = GaussSigma.s0d50;
        public StageGaussianBlur(GpuContext ctx) : base(ctx) {}
        public override void Schedule(PipelineWorkItem requirements, GpuJobHandle dependency) {
            CheckRequirements<GeneratorData>(requirements);
            GeneratorData d = (GeneratorData) requirements.data;
            int width_ = BlurHelper.limitWidth(width);
            ulong h;
            if (d.write != null) {
                NzRwTile t = new NzRwTile { read = d.data.Ptr, write = d.write.Ptr, resolution = d.resolution, count = BatchCount(d) };
                Native.Check(Native.nz_gauss_blur_stage_rw(ctx.Handle, ref t, width_, (int) sigma, iterations, dependency.id, out h), "nz_gauss_blur_stage_rw");
                Adopt(d, t);
            } else if (d is GeneratorDataBatch b) {
                Native.Check(Native.nz_gauss_blur_stage_batch(ctx.Handle, b.data.Ptr, tmp.Ptr, width_, (int) sigma, iterations, b.resolution, b.count, dependency.id, out h), "nz_gauss_blur_stage_batch");
            } else {
                Native.Check(Native.nz_gauss_blur_stage(ctx.Handle, d.data.Ptr, tmp.Ptr, width_, (int) sigma, iterations, d.resolution, dependency.id, out h), "nz_gauss_blur_stage");
            }
            jobHandle = Done(h);
        }
    }

    public class StageSmoothBlur : TmpStage {
        public int iterations = 1, width = 1;
        public StageSmoothBlur(GpuContext ctx) : base(ctx) {}
        public override void Schedule(PipelineWorkItem requirements, GpuJobHandle dependency) {
            CheckRequirements<GeneratorData>(requirements);
            GeneratorData d = (GeneratorData) requirements.data;
            int width_ = BlurHelper.limitWidth(width);
            ulong h;
            if (d.write != null) {
                NzRwTile t = new NzRwTile { read = d.data.Ptr, write = d.write.Ptr, resolution = d.resolution, count = BatchCount(d) };
                Native.Check(Native.nz_smooth_blur_stage_rw(ctx.Handle, ref t, width_, iterations, dependency.id, out h), "nz_smooth_blur_stage_rw");
                Adopt(d, t);
            } else if (d is GeneratorDataBatch b) {
                Native.Check(Native.nz_smooth_blur_stage_batch(ctx.Handle, b.data.Ptr, tmp.Ptr, width_, iterations, b.resolution, b.count, dependency.id, out h), "nz_smooth_blur_stage_batch");
            } else {
                Native.Check(Native.nz_smooth_blur_stage(ctx.Handle, d.data.Ptr, tmp.Ptr, width_, iterations, d.resolution, dependency.id, out h), "nz_smooth_blur_stage");
            }
            jobHandle = Done(h);
        }
    }

    public class ErosionStage : TmpStage {
        public int iterations = 1;
        public ErosionStage(GpuContext ctx) : base(ctx) {}
        public override void Schedule(PipelineWorkItem requirements, GpuJobHandle dependency) {
            CheckRequirements<GeneratorData>(requirements);
            GeneratorData d = (GeneratorData) requirements.data;
            ulong h;
            if (d.write != null) {
                NzRwTile t = new NzRwTile { read = d.data.Ptr, write = d.write.Ptr, resolution = d.resolution, count = BatchCount(d) };
                Native.Check(Native.nz_erosion_stage_rw(ctx.Handle, ref t, iterations, dependency.id, out h), "nz_erosion_stage_rw");
                Adopt(d, t);
            } else if (d is GeneratorDataBatch b) {
                Native.Check(Native.nz_erosion_stage_batch(ctx.Handle, b.data.Ptr, tmp.Ptr, iterations, b.resolution, b.count, dependency.id, out h), "nz_erosion_stage_batch");
            } else {
                Native.Check(Native.nz_erosion_stage(ctx.Handle, d.data.Ptr, tmp.Ptr, iterations, d.resolution, dependency.id, out h), "nz_erosion_stage");
            }
            jobHandle = Done(h);
        }
    }

    public class CropStage : PipelineStage {      // "CenterCropResolution": the job never sets its offset, so the crop is top-left (CropJob.cs:43-59)
        public CropStage(GpuContext ctx) : base(ctx) {}
        public override void Schedule(PipelineWorkItem requirements, GpuJobHandle dependency) {
            if (!(requirements.data is DownsampleData d)) throw new Exception($"Unhandled stageio {requirements.data.GetType()}");
            Native.Check(Native.nz_crop_job(ctx.Handle, d.inputData.Ptr, d.inputResolution, d.data.Ptr, d.resolution, dependency.id, out ulong h), "nz_crop_job");
            jobHandle = Done(h);
        }
    }

    public class StageThermalErosion : PipelineStage {
        public int iterations = 1;
        public float talus = 45f, increment = 0.5f, meshHeightWidthRatio = 0.75f;
        public StageThermalErosion(GpuContext ctx) : base(ctx) {}
        public override void Schedule(PipelineWorkItem requirements, GpuJobHandle dependency) {     // :20-28
            CheckRequirements<GeneratorData>(requirements);
            GeneratorData d = (GeneratorData) requirements.data;
            Native.Check(Native.nz_thermal_erosion(ctx.Handle, d.data.Ptr, talus, increment, meshHeightWidthRatio, iterations, d.resolution,
                                                   dependency.id, out ulong h), "nz_thermal_erosion");
            jobHandle = Done(h);
        }
    }

    public class FlowMapStage : PipelineStage {
        public int iterations = 5;
        public float normMin = -0.1f, normMax = 0.1f;
        DeviceTile work;                         // the stage's water / flux READ + WRITE planes (:52-62)
        public FlowMapStage(GpuContext ctx) : base(ctx) {}
        public override void ResizeNativeContainers(int size) {                                     // :197-205
            work?.Dispose();
            work = ctx.Alloc(11 * size);         // the stage's 11 planes (nz_flowmap_stage_work_floats); a batch stacks its tiles inside every plane
        }
        public override void Schedule(PipelineWorkItem requirements, GpuJobHandle dependency) {     // :207-214 -> ScheduleAll :124-195
            CheckRequirements<GeneratorData>(requirements);
            GeneratorData d = (GeneratorData) requirements.data;
            ulong h;
            if (d.write != null) {
                NzRwTile t = new NzRwTile { read = d.data.Ptr, write = d.write.Ptr, resolution = d.resolution, count = d is GeneratorDataBatch bb ? bb.count : 1 };
                Native.Check(Native.nz_flowmap_stage_rw(ctx.Handle, ref t, work.Ptr, iterations, normMin, normMax, dependency.id, out h), "nz_flowmap_stage_rw");
                Adopt(d, t);
            } else if (d is GeneratorDataBatch b) {
                Native.Check(Native.nz_flowmap_stage_batch(ctx.Handle, b.data.Ptr, work.Ptr, iterations, normMin, normMax, b.resolution, b.count, dependency.id, out h), "nz_flowmap_stage_batch");
            } else {
                Native.Check(Native.nz_flowmap_stage(ctx.Handle, d.data.Ptr, work.Ptr, iterations, normMin, normMax, d.resolution, dependency.id, out h), "nz_flowmap_stage");
            }
            jobHandle = Done(h);
        }
        public override void OnDestroy() { work?.Dispose(); work = null; }                          // :216-219
    }

    // Grid hydraulic erosion with sediment transport (new-framework feature; the model: nz_hydraulic_erosion_stage in
    // include/noize_hip.h).  Owns its work planes like FlowMapStage; once the handle completes, Water holds the final water
    // depth of the last payload (count * resolution^2 floats), a river and lake mask.
    // border = Open lets water and sediment run off the tile; rainMap / hardness are planes of the payload's size the caller
    // supplies and keeps alive (rain * rainMap, dissolve * (1 - hardness)); recordMasks makes the stage own Wear and Deposits.
    // With all four at their defaults the stage calls the plain entries.
    public enum HydraulicBorder { Closed = 0, Open = 1 }                                            // enum nz_hydraulic_border

    public class HydraulicErosionStage : PipelineStage {
        public int iterations = 200;
        public float initialWater = 1e-4f, rain = 1e-4f, evaporation = 0.01f, capacity = 1f, dissolve = 0.3f, deposit = 0.3f, minTilt = 0.01f;
        public HydraulicBorder border = HydraulicBorder.Closed;
        public DeviceTile rainMap = null;
        public DeviceTile hardness = null;
        public bool recordMasks = false;
        DeviceTile work;                         // nz_hydraulic_erosion_work_floats planes; the first count * resolution^2 floats: the water
        DeviceTile masks;                        // recordMasks: wear, then deposits, count * resolution^2 floats each
        int resolution, count = 1;
        public HydraulicErosionStage(GpuContext ctx) : base(ctx) {}
        int Cells => count * resolution * resolution;
        public DeviceTile Water => work?.Offset(0, Cells);
        public DeviceTile Wear => masks?.Offset(0, Cells);
        public DeviceTile Deposits => masks?.Offset(Cells, Cells);
        public override void ResizeNativeContainers(int size) {
            work?.Dispose();
            work = ctx.Alloc((int) (ulong) Native.nz_hydraulic_erosion_work_floats(resolution, count));
            masks?.Dispose();
            masks = recordMasks ? ctx.Alloc(2 * Cells) : null;
        }
        public override void Schedule(PipelineWorkItem requirements, GpuJobHandle dependency) {
            if (requirements.data is GeneratorData g) {
                resolution = g.resolution;
                count = g is GeneratorDataBatch gb ? gb.count : 1;
            }
            CheckRequirements<GeneratorData>(requirements);  // sized on the payload's count * resolution^2 cells
            GeneratorData d = (GeneratorData) requirements.data;
            if (!recordMasks) { masks?.Dispose(); masks = null; }  // switched off after a payload of this length: Wear and Deposits are empty again
            ulong h;
            if (border != HydraulicBorder.Closed || rainMap != null || hardness != null || recordMasks) {
                foreach (DeviceTile m in new[] { rainMap, hardness })   // before any launch
                    if (m != null && m.Length != Cells) throw new Exception($"HydraulicErosionStage: a map of {m.Length} floats does not fit the payload's {Cells}");
                if (recordMasks && (masks == null || masks.Length != 2 * Cells)) ResizeNativeContainers(Cells);
                NzHydraulicDesc desc = new NzHydraulicDesc {
                    iterations = iterations, initialWater = initialWater, rain = rain, evaporation = evaporation, capacity = capacity,
                    dissolve = dissolve, deposit = deposit, minTilt = minTilt, border = (int) border,
                    rainMap = rainMap != null ? rainMap.Ptr : IntPtr.Zero, hardness = hardness != null ? hardness.Ptr : IntPtr.Zero,
                    wear = recordMasks ? Wear.Ptr : IntPtr.Zero, deposits = recordMasks ? Deposits.Ptr : IntPtr.Zero };
                if (d.write != null) {
                    NzRwTile t = new NzRwTile { read = d.data.Ptr, write = d.write.Ptr, resolution = d.resolution, count = count };
                    Native.Check(Native.nz_hydraulic_erosion_ex_rw(ctx.Handle, ref t, work.Ptr, ref desc, dependency.id, out h), "nz_hydraulic_erosion_ex_rw");
                    Adopt(d, t);
                } else if (d is GeneratorDataBatch eb) {
                    Native.Check(Native.nz_hydraulic_erosion_ex_batch(ctx.Handle, eb.data.Ptr, work.Ptr, ref desc, eb.resolution, eb.count, dependency.id, out h), "nz_hydraulic_erosion_ex_batch");
                } else {
                    Native.Check(Native.nz_hydraulic_erosion_ex(ctx.Handle, d.data.Ptr, work.Ptr, ref desc, d.resolution, dependency.id, out h), "nz_hydraulic_erosion_ex");
                }
                jobHandle = Done(h);
                return;
            }
            if (d.write != null) {
                NzRwTile t = new NzRwTile { read = d.data.Ptr, write = d.write.Ptr, resolution = d.resolution, count = count };
                Native.Check(Native.nz_hydraulic_erosion_stage_rw(ctx.Handle, ref t, work.Ptr, iterations, initialWater, rain, evaporation, capacity, dissolve, deposit, minTilt, dependency.id, out h), "nz_hydraulic_erosion_stage_rw");
                Adopt(d, t);
            } else if (d is GeneratorDataBatch b) {
                Native.Check(Native.nz_hydraulic_erosion_stage_batch(ctx.Handle, b.data.Ptr, work.Ptr, iterations, initialWater, rain, evaporation, capacity, dissolve, deposit, minTilt, b.resolution, b.count, dependency.id, out h), "nz_hydraulic_erosion_stage_batch");
            } else {
                Native.Check(Native.nz_hydraulic_erosion_stage(ctx.Handle, d.data.Ptr, work.Ptr, iterations, initialWater, rain, evaporation, capacity, dissolve, deposit, minTilt, d.resolution, dependency.id, out h), "nz_hydraulic_erosion_stage");
            }
            jobHandle = Done(h);
        }
        // The stage on one row stripe of a larger grid (nz_hydraulic_stripe): `n` iterations with this stage's scalars and border in
        // one call; the planes -- all of the stripe's shape -- are the caller's, and so is the exchange of 3 * n ghost rows before
        // the call (Native.nz_halo_exchange on heightIn and, unless `first`, the six stateIn planes).  `maps`: {rainMap, hardness},
        // `masks`: {wear, deposits}, IntPtr.Zero for an option left off.
        public GpuJobHandle ScheduleStripe(IntPtr heightIn, IntPtr heightOut, IntPtr[] stateIn, IntPtr[] stateOut, IntPtr stripeWork,
                                           ref NzStripe st, int n, bool first, bool last, IntPtr[] maps, IntPtr[] masks, GpuJobHandle dependency) {
            NzHydraulicDesc desc = new NzHydraulicDesc {
                iterations = n, initialWater = initialWater, rain = rain, evaporation = evaporation, capacity = capacity,
                dissolve = dissolve, deposit = deposit, minTilt = minTilt, border = (int) border,
                rainMap = maps[0], hardness = maps[1], wear = masks[0], deposits = masks[1] };
            ulong h;
            Native.Check(Native.nz_hydraulic_stripe(ctx.Handle, heightIn, heightOut, stateIn, stateOut, stripeWork, ref st, ref desc, first ? 1 : 0, last ? 1 : 0, dependency.id, out h), "nz_hydraulic_stripe");
            return Done(h);
        }
        public override void OnDestroy() { work?.Dispose(); work = null; masks?.Dispose(); masks = null; }
    }

    // Stream-power fluvial erosion with drainage area (new-framework feature; the model: nz_fluvial_erosion in
    // include/noize_hip.h): dendritic valleys that run from the ridges to the tile's border.  Owns its work planes like
    // HydraulicErosionStage; once the handle completes, Drainage holds the drainage area of the last payload (count *
    // resolution^2 floats), the river map.  seaLevel: cells at or below it are outlets like the border (-float.MaxValue: off).
    // rainMap / hardness / upliftMap / drainageIn are planes of the payload's size the caller supplies and keeps alive
    // (rain * rainMap, erodibility * (1 - hardness), uplift * upliftMap, the drainage to start from).
    public class FluvialErosionStage : PipelineStage {
        public int iterations = 200;
        public float erodibility = 0.05f, uplift = 0.002f, dt = 1f, rain = 1f, seaLevel = -float.MaxValue;
        public DeviceTile rainMap = null;
        public DeviceTile hardness = null;
        public DeviceTile upliftMap = null;
        public DeviceTile drainageIn = null;
        DeviceTile work;                         // nz_fluvial_erosion_work_floats planes; the first count * resolution^2 floats: the drainage
        int resolution, count = 1;
        public FluvialErosionStage(GpuContext ctx) : base(ctx) {}
        int Cells => count * resolution * resolution;
        public DeviceTile Drainage => work?.Offset(0, Cells);
        public override void ResizeNativeContainers(int size) {
            work?.Dispose();
            work = ctx.Alloc((int) (ulong) Native.nz_fluvial_erosion_work_floats(resolution, count));
        }
        public override void Schedule(PipelineWorkItem requirements, GpuJobHandle dependency) {
            if (requirements.data is GeneratorData g) {
                resolution = g.resolution;
                count = g is GeneratorDataBatch gb ? gb.count : 1;
            }
            CheckRequirements<GeneratorData>(requirements);  // sized on the payload's count * resolution^2 cells
            GeneratorData d = (GeneratorData) requirements.data;
            foreach (DeviceTile m in new[] { rainMap, hardness, upliftMap, drainageIn })   // before any launch
                if (m != null && m.Length != Cells) throw new Exception($"FluvialErosionStage: a plane of {m.Length} floats does not fit the payload's {Cells}");
            NzFluvialDesc desc = new NzFluvialDesc {
                iterations = iterations, erodibility = erodibility, uplift = uplift, dt = dt, rain = rain, seaLevel = seaLevel,
                rainMap = rainMap != null ? rainMap.Ptr : IntPtr.Zero, hardness = hardness != null ? hardness.Ptr : IntPtr.Zero,
                upliftMap = upliftMap != null ? upliftMap.Ptr : IntPtr.Zero, drainageIn = drainageIn != null ? drainageIn.Ptr : IntPtr.Zero };
            ulong h;
            if (d.write != null) {
                NzRwTile t = new NzRwTile { read = d.data.Ptr, write = d.write.Ptr, resolution = d.resolution, count = count };
                Native.Check(Native.nz_fluvial_erosion_rw(ctx.Handle, ref t, work.Ptr, ref desc, dependency.id, out h), "nz_fluvial_erosion_rw");
                Adopt(d, t);
            } else if (d is GeneratorDataBatch b) {
                Native.Check(Native.nz_fluvial_erosion_batch(ctx.Handle, b.data.Ptr, work.Ptr, ref desc, b.resolution, b.count, dependency.id, out h), "nz_fluvial_erosion_batch");
            } else {
                Native.Check(Native.nz_fluvial_erosion(ctx.Handle, d.data.Ptr, work.Ptr, ref desc, d.resolution, dependency.id, out h), "nz_fluvial_erosion");
            }
            jobHandle = Done(h);
        }
        // The stage on one row stripe of a larger grid (nz_fluvial_stripe): `n` iterations with this stage's scalars in one call;
        // the planes -- all of the stripe's shape -- are the caller's, and so is the exchange of 2 * n ghost rows before the call
        // (Native.nz_halo_exchange on heightIn and, when given, drainageInRows; the maps once, before the first call).
        // IntPtr.Zero for a map is an option left off; drainageInRows Zero: the start state.
        public GpuJobHandle ScheduleStripe(IntPtr heightIn, IntPtr heightOut, IntPtr drainageOut, IntPtr stripeWork, ref NzStripe st,
                                           int n, IntPtr drainageInRows, IntPtr rainMapRows, IntPtr hardnessRows, IntPtr upliftMapRows,
                                           GpuJobHandle dependency) {
            NzFluvialDesc desc = new NzFluvialDesc {
                iterations = n, erodibility = erodibility, uplift = uplift, dt = dt, rain = rain, seaLevel = seaLevel,
                rainMap = rainMapRows, hardness = hardnessRows, upliftMap = upliftMapRows, drainageIn = drainageInRows };
            ulong h;
            Native.Check(Native.nz_fluvial_stripe(ctx.Handle, heightIn, heightOut, drainageOut, stripeWork, ref st, ref desc, dependency.id, out h), "nz_fluvial_stripe");
            return Done(h);
        }
        public override void OnDestroy() { work?.Dispose(); work = null; }
    }

    // Depression filling (new-framework feature; the model: nz_fill_depressions in include/noize_hip.h): every closed hollow
    // is raised to its spill level plus an epsilon gradient, so that FluvialErosionStage's river network reaches the border
    // from its first iteration.  Owns its work planes like FluvialErosionStage.  With recordDepth, Depth holds the lake depth
    // of the last payload (count * resolution^2 floats; zero where nothing was filled) once the handle completes; Passes and
    // Converged wait for the handle and read the status words.  seaLevel: cells at or below it are outlets like the border
    // (-float.MaxValue: off).  maxPasses null means the default, 64 + resolution / 4; a budget that runs out is no error:
    // Converged is false, the heights are as they were and the depth is zero.
    public class DepressionFillStage : PipelineStage {
        public float epsilon = 1e-4f, seaLevel = -float.MaxValue;
        public int? maxPasses = null;
        public bool recordDepth = false;
        DeviceTile work;                         // nz_fill_depressions_work_floats floats; its first two int32: {passes, converged}
        DeviceTile lakes;
        int resolution, count = 1;
        public DepressionFillStage(GpuContext ctx) : base(ctx) {}
        int Cells => count * resolution * resolution;
        public DeviceTile Depth => lakes;
        public int? Passes => Status(0);
        public bool? Converged => Status(1) is int c ? c == 1 : (bool?) null;
        int? Status(int k) {
            if (work == null) return null;
            jobHandle.Complete();
            return BitConverter.SingleToInt32Bits(work.Offset(0, 2).ToArray()[k]);
        }
        public override void Schedule(PipelineWorkItem requirements, GpuJobHandle dependency) {
            if (requirements.data is GeneratorData g) {
                resolution = g.resolution;
                count = g is GeneratorDataBatch gb ? gb.count : 1;
            }
            CheckRequirements<GeneratorData>(requirements);
            GeneratorData d = (GeneratorData) requirements.data;
            // sized on (resolution, count), not on the payload's cell count alone: the per-tile bytes depend on the number
            // of 64 x 16 tiles, so two payloads of equal length can need different sizes
            int need = (int) (ulong) Native.nz_fill_depressions_work_floats(resolution, count);
            if (work == null || work.Length != need) { work?.Dispose(); work = ctx.Alloc(need); }
            if (!recordDepth || (lakes != null && lakes.Length != Cells)) { lakes?.Dispose(); lakes = null; }
            if (recordDepth && lakes == null) lakes = ctx.Alloc(Cells);
            NzFillDesc desc = new NzFillDesc {
                epsilon = epsilon, seaLevel = seaLevel, maxPasses = maxPasses ?? 64 + resolution / 4,
                depth = lakes != null ? lakes.Ptr : IntPtr.Zero };
            ulong h;
            if (d.write != null) {
                NzRwTile t = new NzRwTile { read = d.data.Ptr, write = d.write.Ptr, resolution = d.resolution, count = count };
                Native.Check(Native.nz_fill_depressions_rw(ctx.Handle, ref t, work.Ptr, ref desc, dependency.id, out h), "nz_fill_depressions_rw");
                Adopt(d, t);
            } else if (d is GeneratorDataBatch b) {
                Native.Check(Native.nz_fill_depressions_batch(ctx.Handle, b.data.Ptr, work.Ptr, ref desc, b.resolution, b.count, dependency.id, out h), "nz_fill_depressions_batch");
            } else {
                Native.Check(Native.nz_fill_depressions(ctx.Handle, d.data.Ptr, work.Ptr, ref desc, d.resolution, dependency.id, out h), "nz_fill_depressions");
            }
            jobHandle = Done(h);
        }
        // The stage on one row stripe of a larger grid, one round (nz_fill_stripe): at most `passes` passes with this stage's
        // epsilon and sea level over the owned rows, against one frozen ghost row of W on each side.  The planes and words are
        // the caller's (stripeWork: Native.nz_fill_stripe_work_floats), and so are the exchange of one row before the call -- of
        // heightRows before the round with `first`, of wRows before every later one -- and the vote after it
        // (Native.nz_comm_allreduce_max_i32 on `changed`, which the next round takes as its `proceed`; IntPtr.Zero in the first).
        public GpuJobHandle ScheduleStripe(IntPtr heightRows, IntPtr wRows, IntPtr stripeWork, ref NzStripe st, int passes, bool first,
                                           IntPtr proceed, IntPtr changed, GpuJobHandle dependency) {
            NzFillDesc desc = new NzFillDesc { epsilon = epsilon, seaLevel = seaLevel, maxPasses = passes, depth = IntPtr.Zero };
            ulong h;
            Native.Check(Native.nz_fill_stripe(ctx.Handle, heightRows, wRows, stripeWork, ref st, ref desc, first ? 1 : 0, proceed, changed, dependency.id, out h), "nz_fill_stripe");
            return Done(h);
        }
        // ... and the end of the rounds (nz_fill_stripe_finalise): all or nothing on the owned rows by the device word
        // `converged`, the verdict "the last vote was 0"; depthRows may be IntPtr.Zero.
        public GpuJobHandle FinaliseStripe(IntPtr heightRows, IntPtr wRows, IntPtr depthRows, ref NzStripe st, IntPtr converged, GpuJobHandle dependency) {
            ulong h;
            Native.Check(Native.nz_fill_stripe_finalise(ctx.Handle, heightRows, wRows, depthRows, ref st, converged, dependency.id, out h), "nz_fill_stripe_finalise");
            return Done(h);
        }
        public override void OnDestroy() { work?.Dispose(); work = null; lakes?.Dispose(); lakes = null; }
    }

    // Drainage area (new-framework feature; the model: nz_drainage_area in include/noize_hip.h): the exact flow accumulation
    // over the steepest-descent tree of the payload's heights -- the river map -- in one call.  The heights pass through
    // untouched.  Once the handle completes, Drainage holds the plane of the last payload (count * resolution^2 floats);
    // Passes and Converged wait for the handle and read the status words.  seaLevel: cells at or below it are outlets like
    // the border (-float.MaxValue: off).  rainMap: a plane of the payload's size the caller supplies and keeps alive.
    // maxPasses null means the default, 64 + resolution / 4; a budget that runs out is no error: Converged is false and the
    // drainage is the start state.  @out: a caller-supplied plane of the payload's size that receives the drainage -- the plane
    // FluvialErosionStage.drainageIn takes; without it the stage owns the plane.
    public class DrainageAreaStage : PipelineStage {
        public float rain = 1f, seaLevel = -float.MaxValue;
        public int? maxPasses = null;
        public DeviceTile rainMap = null;
        public DeviceTile @out = null;
        DeviceTile work;                         // nz_drainage_area_work_floats floats; its first two int32: {passes, converged}
        DeviceTile plane;
        int resolution, count = 1;
        public DrainageAreaStage(GpuContext ctx) : base(ctx) {}
        int Cells => count * resolution * resolution;
        public DeviceTile Drainage => work == null ? null : @out ?? plane;
        public int? Passes => Status(0);
        public bool? Converged => Status(1) is int c ? c == 1 : (bool?) null;
        int? Status(int k) {
            if (work == null) return null;
            jobHandle.Complete();
            return BitConverter.SingleToInt32Bits(work.Offset(0, 2).ToArray()[k]);
        }
        public override void Schedule(PipelineWorkItem requirements, GpuJobHandle dependency) {
            if (requirements.data is GeneratorData g) {
                resolution = g.resolution;
                count = g is GeneratorDataBatch gb ? gb.count : 1;
            }
            CheckRequirements<GeneratorData>(requirements);
            GeneratorData d = (GeneratorData) requirements.data;
            foreach (DeviceTile m in new[] { rainMap, @out })   // before any launch
                if (m != null && m.Length != Cells) throw new Exception($"DrainageAreaStage: a plane of {m.Length} floats does not fit the payload's {Cells}");
            // sized on (resolution, count) like DepressionFillStage's: the per-tile bytes depend on the number of 64 x 16 tiles
            int need = (int) (ulong) Native.nz_drainage_area_work_floats(resolution, count);
            if (work == null || work.Length != need) { work?.Dispose(); work = ctx.Alloc(need); }
            if (@out != null || (plane != null && plane.Length != Cells)) { plane?.Dispose(); plane = null; }
            if (@out == null && plane == null) plane = ctx.Alloc(Cells);
            NzDrainageDesc desc = new NzDrainageDesc {
                rain = rain, seaLevel = seaLevel, maxPasses = maxPasses ?? 64 + resolution / 4,
                rainMap = rainMap != null ? rainMap.Ptr : IntPtr.Zero };
            IntPtr dst = (@out ?? plane).Ptr;
            ulong h;
            if (d is GeneratorDataBatch b) {
                Native.Check(Native.nz_drainage_area_batch(ctx.Handle, b.data.Ptr, dst, work.Ptr, ref desc, b.resolution, b.count, dependency.id, out h), "nz_drainage_area_batch");
            } else {
                Native.Check(Native.nz_drainage_area(ctx.Handle, d.data.Ptr, dst, work.Ptr, ref desc, d.resolution, dependency.id, out h), "nz_drainage_area");
            }
            jobHandle = Done(h);
        }
        // The stage on one row stripe of a larger grid, one round (nz_drainage_stripe_round): at most `passes` passes with this stage's
        // rain and sea level over the owned rows, against one frozen ghost row of A on each side.  The planes and words are the
        // caller's (stripeWork: Native.nz_drainage_stripe_work_floats; rainMapRows may be IntPtr.Zero), and so are the exchange
        // before the call -- 2 rows of heightRows and of rainMapRows before the round with `first`, 1 row of aRows before every
        // later one -- and the vote after it (Native.nz_comm_allreduce_max_i32 on `changed`, which the next round takes as its
        // `proceed`; IntPtr.Zero in the first).
        public GpuJobHandle ScheduleStripe(IntPtr heightRows, IntPtr aRows, IntPtr stripeWork, IntPtr rainMapRows, ref NzStripe st, int passes,
                                           bool first, IntPtr proceed, IntPtr changed, GpuJobHandle dependency) {
            NzDrainageDesc desc = new NzDrainageDesc { rain = rain, seaLevel = seaLevel, maxPasses = passes, rainMap = rainMapRows };
            ulong h;
            Native.Check(Native.nz_drainage_stripe_round(ctx.Handle, heightRows, aRows, stripeWork, ref st, ref desc, first ? 1 : 0, proceed, changed, dependency.id, out h), "nz_drainage_stripe_round");
            return Done(h);
        }
        // ... and the end of the rounds (nz_drainage_stripe_finalise): all or nothing on the owned rows by the device word
        // `converged`, the verdict "the last vote was 0".  aRows then serves FluvialErosionStage's stripe form as its drainageIn.
        public GpuJobHandle FinaliseStripe(IntPtr aRows, IntPtr rainMapRows, ref NzStripe st, IntPtr converged, GpuJobHandle dependency) {
            NzDrainageDesc desc = new NzDrainageDesc { rain = rain, seaLevel = seaLevel, maxPasses = 1, rainMap = rainMapRows };
            ulong h;
            Native.Check(Native.nz_drainage_stripe_finalise(ctx.Handle, aRows, ref st, ref desc, converged, dependency.id, out h), "nz_drainage_stripe_finalise");
            return Done(h);
        }
        public override void OnDestroy() { work?.Dispose(); work = null; plane?.Dispose(); plane = null; }
    }

    // How ImplicitFluvialStage routes the drainage area: Steepest gives all of a cell's water to its steepest neighbour
    // (DrainageAreaStage's rule), Multiple a slope-weighted share to every lower neighbour (MfdDrainageStage's).
    public enum FlowRouting { Steepest = 0, Multiple = 1 }

    // Multiple-flow drainage (new-framework feature; the model: nz_drainage_mfd in include/noize_hip.h): the flow accumulation
    // of the payload's heights with every lower neighbour taking the share (slope / steepest slope) ^ exponent of a cell's
    // water, normalised -- no parallel one-cell lines on hillsides, and water spreads on fans.  In every other respect the
    // stage is DrainageAreaStage: the heights pass through, Drainage, Passes and Converged describe the last payload,
    // seaLevel, rainMap and @out mean the same, a budget that runs out is no error and leaves the start state.  exponent:
    // 1..16; 1 spreads most, larger values approach DrainageAreaStage.  maxPasses null means the default,
    // 128 + resolution / 2, twice DrainageAreaStage's: the flow graph's paths are longer than the tree's.  The entry has no
    // row-stripe form.
    public class MfdDrainageStage : PipelineStage {
        public float rain = 1f, seaLevel = -float.MaxValue;
        public int exponent = 1;
        public int? maxPasses = null;
        public DeviceTile rainMap = null;
        public DeviceTile @out = null;
        DeviceTile work;                         // nz_drainage_mfd_work_floats floats; its first two int32: {passes, converged}
        DeviceTile plane;
        int resolution, count = 1;
        public MfdDrainageStage(GpuContext ctx) : base(ctx) {}
        int Cells => count * resolution * resolution;
        public DeviceTile Drainage => work == null ? null : @out ?? plane;
        public int? Passes => Status(0);
        public bool? Converged => Status(1) is int c ? c == 1 : (bool?) null;
        int? Status(int k) {
            if (work == null) return null;
            jobHandle.Complete();
            return BitConverter.SingleToInt32Bits(work.Offset(0, 2).ToArray()[k]);
        }
        public override void Schedule(PipelineWorkItem requirements, GpuJobHandle dependency) {
            if (requirements.data is GeneratorData g) {
                resolution = g.resolution;
                count = g is GeneratorDataBatch gb ? gb.count : 1;
            }
            CheckRequirements<GeneratorData>(requirements);
            GeneratorData d = (GeneratorData) requirements.data;
            foreach (DeviceTile m in new[] { rainMap, @out })   // before any launch
                if (m != null && m.Length != Cells) throw new Exception($"MfdDrainageStage: a plane of {m.Length} floats does not fit the payload's {Cells}");
            // sized on (resolution, count) like DrainageAreaStage's: the per-tile bytes depend on the number of 64 x 16 tiles
            int need = (int) (ulong) Native.nz_drainage_mfd_work_floats(resolution, count);
            if (work == null || work.Length != need) { work?.Dispose(); work = ctx.Alloc(need); }
            if (@out != null || (plane != null && plane.Length != Cells)) { plane?.Dispose(); plane = null; }
            if (@out == null && plane == null) plane = ctx.Alloc(Cells);
            NzDrainageMfdDesc desc = new NzDrainageMfdDesc {
                rain = rain, seaLevel = seaLevel, maxPasses = maxPasses ?? 128 + resolution / 2, exponent = exponent,
                rainMap = rainMap != null ? rainMap.Ptr : IntPtr.Zero };
            IntPtr dst = (@out ?? plane).Ptr;
            ulong h;
            if (d is GeneratorDataBatch b) {
                Native.Check(Native.nz_drainage_mfd_batch(ctx.Handle, b.data.Ptr, dst, work.Ptr, ref desc, b.resolution, b.count, dependency.id, out h), "nz_drainage_mfd_batch");
            } else {
                Native.Check(Native.nz_drainage_mfd(ctx.Handle, d.data.Ptr, dst, work.Ptr, ref desc, d.resolution, dependency.id, out h), "nz_drainage_mfd");
            }
            jobHandle = Done(h);
        }
        public override void OnDestroy() { work?.Dispose(); work = null; plane?.Dispose(); plane = null; }
    }

    // Watershed (new-framework feature; the model: nz_watershed in include/noize_hip.h): the steepest-descent tree of the
    // payload's heights read upstream -- which outlet or pit every cell drains to, how far along the river it lies, and the
    // tree itself.  The heights pass through untouched.  Once the handle completes, Basin holds the labels of the last payload
    // (count * resolution^2 int32 in four-byte cells: BitConverter.SingleToInt32Bits; the index of the outlet or pit inside
    // the cell's own tile), Length the flow-path length to it and Receivers one code per cell (0..7 in the order W E S N SW SE
    // NW NE, 8 without a receiver; four codes per cell of the tile); Passes and Converged wait for the handle and read the
    // status words.  seaLevel: cells at or below it are outlets like the border (-float.MaxValue: off).  cellSize: the length
    // of a straight move.  maxPasses null means the default, 64 + resolution / 4; a budget that runs out is no error:
    // Converged is false, the labels are the cells' own indices and the length is zero.  length = false: labels only.
    // recordReceivers: keep the receiver plane.
    public class WatershedStage : PipelineStage {
        public float seaLevel = -float.MaxValue, cellSize = 1f;
        public int? maxPasses = null;
        public bool length = true;
        public bool recordReceivers = false;
        DeviceTile work;                         // nz_watershed_work_floats floats; its first two int32: {passes, converged}
        DeviceTile labels, lengths, codes;
        int resolution, count = 1;
        public WatershedStage(GpuContext ctx) : base(ctx) {}
        int Cells => count * resolution * resolution;
        public DeviceTile Basin => labels;
        public DeviceTile Length => lengths;
        public DeviceTile Receivers => codes;
        public int? Passes => Status(0);
        public bool? Converged => Status(1) is int c ? c == 1 : (bool?) null;
        int? Status(int k) {
            if (work == null) return null;
            jobHandle.Complete();
            return BitConverter.SingleToInt32Bits(work.Offset(0, 2).ToArray()[k]);
        }
        DeviceTile Size(DeviceTile t, bool want, int n) {   // a plane of the stage: resized with the payload, gone when not wanted
            if (t != null && (!want || t.Length != n)) { t.Dispose(); t = null; }
            return want && t == null ? ctx.Alloc(n) : t;
        }
        public override void Schedule(PipelineWorkItem requirements, GpuJobHandle dependency) {
            if (requirements.data is GeneratorData g) {
                resolution = g.resolution;
                count = g is GeneratorDataBatch gb ? gb.count : 1;
            }
            CheckRequirements<GeneratorData>(requirements);
            GeneratorData d = (GeneratorData) requirements.data;
            // sized on (resolution, count) like DepressionFillStage's: the per-tile bytes depend on the number of 64 x 16 tiles
            int need = (int) (ulong) Native.nz_watershed_work_floats(resolution, count, length ? 1 : 0);
            if (work == null || work.Length != need) { work?.Dispose(); work = ctx.Alloc(need); }
            labels = Size(labels, true, Cells);
            lengths = Size(lengths, length, Cells);
            codes = Size(codes, recordReceivers, (Cells + 3) / 4);   // one byte per cell
            NzWatershedDesc desc = new NzWatershedDesc { seaLevel = seaLevel, cellSize = cellSize, maxPasses = maxPasses ?? 64 + resolution / 4 };
            IntPtr l = lengths != null ? lengths.Ptr : IntPtr.Zero, r = codes != null ? codes.Ptr : IntPtr.Zero;
            ulong h;
            if (d is GeneratorDataBatch b) {
                Native.Check(Native.nz_watershed_batch(ctx.Handle, b.data.Ptr, labels.Ptr, l, r, work.Ptr, ref desc, b.resolution, b.count, dependency.id, out h), "nz_watershed_batch");
            } else {
                Native.Check(Native.nz_watershed(ctx.Handle, d.data.Ptr, labels.Ptr, l, r, work.Ptr, ref desc, d.resolution, dependency.id, out h), "nz_watershed");
            }
            jobHandle = Done(h);
        }
        public override void OnDestroy() {
            work?.Dispose(); work = null; labels?.Dispose(); labels = null; lengths?.Dispose(); lengths = null; codes?.Dispose(); codes = null;
        }
    }

    // Stream order (new-framework feature; the model: nz_stream_order in include/noize_hip.h): the channel cells of the
    // payload's heights, their Strahler order and the unbranched reaches between heads and confluences.  The heights pass
    // through untouched.  Once the handle completes, Order holds one byte per cell of the last payload (0: no channel, 1: a
    // head reach, +1 where two reaches of the same order meet; four orders per cell of the tile) and Links the cell index,
    // inside the cell's own tile, of the head or confluence its reach starts at (count * resolution^2 int32 in four-byte
    // cells: BitConverter.SingleToInt32Bits; -1: no channel); Passes and Converged wait for the handle and read the status
    // words.  seaLevel: cells at or below it are outlets like the border (-float.MaxValue: off).  drainage: a device plane
    // of the payload's size the caller supplies and keeps alive, the one DrainageAreaStage.@out received; a cell is a channel
    // cell when its drainage >= threshold; null: every cell is one.  maxPasses null means the default,
    // 64 + resolution / 4; a budget that runs out is no error: Converged is false, the order is 1 on channel cells and every
    // channel cell is its own link.  recordLinks: carry the link plane.  Strahler streams, as opposed to links, are the
    // caller's to derive from the two planes.
    public class StreamOrderStage : PipelineStage {
        public float seaLevel = -float.MaxValue, threshold = 0f;
        public int? maxPasses = null;
        public DeviceTile drainage = null;
        public bool recordLinks = false;
        DeviceTile work;                         // nz_stream_order_work_floats floats; its first two int32: {passes, converged}
        DeviceTile orders, linkPlane;
        int resolution, count = 1;
        public StreamOrderStage(GpuContext ctx) : base(ctx) {}
        int Cells => count * resolution * resolution;
        public DeviceTile Order => orders;
        public DeviceTile Links => linkPlane;
        public int? Passes => Status(0);
        public bool? Converged => Status(1) is int c ? c == 1 : (bool?) null;
        int? Status(int k) {
            if (work == null) return null;
            jobHandle.Complete();
            return BitConverter.SingleToInt32Bits(work.Offset(0, 2).ToArray()[k]);
        }
        DeviceTile Size(DeviceTile t, bool want, int n) {   // a plane of the stage: resized with the payload, gone when not wanted
            if (t != null && (!want || t.Length != n)) { t.Dispose(); t = null; }
            return want && t == null ? ctx.Alloc(n) : t;
        }
        public override void Schedule(PipelineWorkItem requirements, GpuJobHandle dependency) {
            if (requirements.data is GeneratorData g) {
                resolution = g.resolution;
                count = g is GeneratorDataBatch gb ? gb.count : 1;
            }
            CheckRequirements<GeneratorData>(requirements);
            GeneratorData d = (GeneratorData) requirements.data;
            if (drainage != null && drainage.Length != Cells)   // before any launch
                throw new Exception($"StreamOrderStage: a drainage plane of {drainage.Length} floats does not fit the payload's {Cells}");
            // sized on (resolution, count) like DepressionFillStage's: the per-tile bytes depend on the number of 64 x 16 tiles
            int need = (int) (ulong) Native.nz_stream_order_work_floats(resolution, count, recordLinks ? 1 : 0);
            if (work == null || work.Length != need) { work?.Dispose(); work = ctx.Alloc(need); }
            orders = Size(orders, true, (Cells + 3) / 4);   // one byte per cell
            linkPlane = Size(linkPlane, recordLinks, Cells);
            NzStreamOrderDesc desc = new NzStreamOrderDesc {
                seaLevel = seaLevel, threshold = threshold, maxPasses = maxPasses ?? 64 + resolution / 4,
                drainage = drainage != null ? drainage.Ptr : IntPtr.Zero };
            IntPtr l = linkPlane != null ? linkPlane.Ptr : IntPtr.Zero;
            ulong h;
            if (d is GeneratorDataBatch b) {
                Native.Check(Native.nz_stream_order_batch(ctx.Handle, b.data.Ptr, orders.Ptr, l, work.Ptr, ref desc, b.resolution, b.count, dependency.id, out h), "nz_stream_order_batch");
            } else {
                Native.Check(Native.nz_stream_order(ctx.Handle, d.data.Ptr, orders.Ptr, l, work.Ptr, ref desc, d.resolution, dependency.id, out h), "nz_stream_order");
            }
            jobHandle = Done(h);
        }
        public override void OnDestroy() {
            work?.Dispose(); work = null; orders?.Dispose(); orders = null; linkPlane?.Dispose(); linkPlane = null;
        }
    }

    // Implicit stream-power fluvial erosion (new-framework feature; the model: nz_fluvial_implicit in include/noize_hip.h):
    // FluvialErosionStage's model taken with the implicit Euler step along the receiver tree -- stable for every dt, so one
    // iteration carries a time step the explicit stage needs hundreds of launches for.  Per iteration the stage computes the
    // exact drainage area of the current heights (nz_drainage_area, into its own plane) and solves the step
    // (nz_fluvial_implicit), told to proceed by the drainage call's converged word on the device; nothing is read back in
    // between.  Pits stay pits: put DepressionFillStage in front.  The heights ping-pong between the payload's plane and its
    // WRITE plane (or a plane of the stage's); the result is in the payload's `data` when the handle completes.  seaLevel:
    // cells at or below it are outlets like the border (-float.MaxValue: off).  rainMap / hardness / upliftMap: device
    // planes of the payload's size the caller keeps alive.  maxPasses null means the default, 64 + resolution / 4, for the
    // drainage series and for the solve each; a budget that runs out is no error: that iteration leaves the heights as they
    // were.  Drainage is the area the last iteration saw; Steps, Passes and Converged wait for the handle and read the
    // stage's tally: the iterations applied, the solve passes that did work, and Steps == iterations.  routing:
    // FlowRouting.Multiple makes the drainage call of every iteration nz_drainage_mfd with flowExponent (1..16), chained
    // through the same proceed word, its default budget 128 + resolution / 2; the solve still lowers each cell along its
    // steepest receiver, only the area changes.
    public class ImplicitFluvialStage : PipelineStage {
        public int iterations = 1;
        public float erodibility = 0.05f, uplift = 0.002f, dt = 1f, rain = 1f, seaLevel = -float.MaxValue;
        public int? maxPasses = null;
        public DeviceTile rainMap = null, hardness = null, upliftMap = null;
        public FlowRouting routing = FlowRouting.Steepest;
        public int flowExponent = 1;
        protected DeviceTile work;               // nz_fluvial_implicit_work_floats floats (a deriving stage: its own entry's)
        DeviceTile drainageWork;                 // the drainage entry's work floats; its second int32: the solve's `proceed`
        protected DeviceTile area;               // the drainage
        DeviceTile plane, tally;                 // the heights' second plane, {steps applied, passes that did work}
        protected int resolution, count = 1;
        static readonly IntPtr Zeros = ZeroWords();   // what the tally is set to before a run; lives as long as the process
        static IntPtr ZeroWords() {
            IntPtr p = System.Runtime.InteropServices.Marshal.AllocHGlobal(8);
            System.Runtime.InteropServices.Marshal.WriteInt64(p, 0L);
            return p;
        }
        public ImplicitFluvialStage(GpuContext ctx) : base(ctx) {}
        protected int Cells => count * resolution * resolution;
        public DeviceTile Drainage => area;
        public int? Steps => Counted(0);
        public int? Passes => Counted(1);
        public bool? Converged => Counted(0) is int s ? s == iterations : (bool?) null;
        int? Counted(int k) {
            if (tally == null) return null;
            jobHandle.Complete();
            return BitConverter.SingleToInt32Bits(tally.ToArray()[k]);
        }
        protected DeviceTile Size(DeviceTile t, bool want, int n) {   // a plane of the stage: resized with the payload, gone when not wanted
            if (t != null && (!want || t.Length != n)) { t.Dispose(); t = null; }
            return want && t == null ? ctx.Alloc(n) : t;
        }
        // the hook of a stage that derives from this one (SedimentFluvialStage): the size of `work`, and the solve of one
        // iteration, heights cur -> other, with the desc of the run
        protected virtual int SolveWorkFloats() => (int) (ulong) Native.nz_fluvial_implicit_work_floats(resolution, count);
        protected virtual void EnqueueSolve(bool batch, DeviceTile cur, DeviceTile other, ref NzFluvialImplicitDesc solve, out ulong h) {
            if (batch) {
                Native.Check(Native.nz_fluvial_implicit_batch(ctx.Handle, cur.Ptr, area.Ptr, other.Ptr, work.Ptr, ref solve, resolution, count, 0, out h), "nz_fluvial_implicit_batch");
            } else {
                Native.Check(Native.nz_fluvial_implicit(ctx.Handle, cur.Ptr, area.Ptr, other.Ptr, work.Ptr, ref solve, resolution, 0, out h), "nz_fluvial_implicit");
            }
        }
        public override void Schedule(PipelineWorkItem requirements, GpuJobHandle dependency) {
            if (requirements.data is GeneratorData g) {
                resolution = g.resolution;
                count = g is GeneratorDataBatch gb ? gb.count : 1;
            }
            CheckRequirements<GeneratorData>(requirements);
            GeneratorData d = (GeneratorData) requirements.data;
            foreach (DeviceTile m in new[] { rainMap, hardness, upliftMap })   // before any launch
                if (m != null && m.Length != Cells) throw new Exception($"ImplicitFluvialStage: a plane of {m.Length} floats does not fit the payload's {Cells}");
            // sized on (resolution, count) like DrainageAreaStage's: the per-tile bytes depend on the number of 64 x 16 tiles
            work = Size(work, true, SolveWorkFloats());
            bool multiple = routing == FlowRouting.Multiple;
            drainageWork = Size(drainageWork, true, (int) (ulong) (multiple ? Native.nz_drainage_mfd_work_floats(resolution, count)
                                                                            : Native.nz_drainage_area_work_floats(resolution, count)));
            area = Size(area, true, Cells);
            plane = Size(plane, d.write == null, Cells);
            tally = Size(tally, true, 2);
            int budget = maxPasses ?? 64 + resolution / 4;
            NzDrainageDesc drain = new NzDrainageDesc {
                rain = rain, seaLevel = seaLevel, maxPasses = budget, rainMap = rainMap != null ? rainMap.Ptr : IntPtr.Zero };
            NzDrainageMfdDesc spread = new NzDrainageMfdDesc {
                rain = rain, seaLevel = seaLevel, maxPasses = maxPasses ?? 128 + resolution / 2, exponent = flowExponent,
                rainMap = rainMap != null ? rainMap.Ptr : IntPtr.Zero };
            NzFluvialImplicitDesc solve = new NzFluvialImplicitDesc {
                erodibility = erodibility, uplift = uplift, dt = dt, seaLevel = seaLevel, maxPasses = budget,
                hardness = hardness != null ? hardness.Ptr : IntPtr.Zero, upliftMap = upliftMap != null ? upliftMap.Ptr : IntPtr.Zero,
                proceed = IntPtr.Add(drainageWork.Ptr, 4), tally = tally.Ptr };
            ulong h;
            Native.Check(Native.nz_tile_upload(ctx.Handle, tally.Ptr, Zeros, (UIntPtr) 2u, dependency.id, out h), "nz_tile_upload");
            // the heights ping-pong between the payload's plane and the WRITE plane (or the stage's own)
            DeviceTile cur = d.data, other = d.write ?? plane;
            bool batch = d is GeneratorDataBatch;
            for (int i = 0; i < iterations; i++) {
                if (multiple && batch) {
                    Native.Check(Native.nz_drainage_mfd_batch(ctx.Handle, cur.Ptr, area.Ptr, drainageWork.Ptr, ref spread, resolution, count, 0, IntPtr.Zero), "nz_drainage_mfd_batch");
                } else if (multiple) {
                    Native.Check(Native.nz_drainage_mfd(ctx.Handle, cur.Ptr, area.Ptr, drainageWork.Ptr, ref spread, resolution, 0, IntPtr.Zero), "nz_drainage_mfd");
                } else if (batch) {
                    Native.Check(Native.nz_drainage_area_batch(ctx.Handle, cur.Ptr, area.Ptr, drainageWork.Ptr, ref drain, resolution, count, 0, IntPtr.Zero), "nz_drainage_area_batch");
                } else {
                    Native.Check(Native.nz_drainage_area(ctx.Handle, cur.Ptr, area.Ptr, drainageWork.Ptr, ref drain, resolution, 0, IntPtr.Zero), "nz_drainage_area");
                }
                EnqueueSolve(batch, cur, other, ref solve, out h);
                DeviceTile s = cur; cur = other; other = s;
            }
            if (d.write != null) { d.data = cur; d.write = other; }   // the pair as the run left it: `data` holds the result
            else if (cur != d.data)                                   // an odd count ended in the stage's plane
                Native.Check(Native.nz_flush_write_slice(ctx.Handle, d.data.Ptr, cur.Ptr, (UIntPtr) (uint) Cells, 0, out h), "nz_flush_write_slice");
            jobHandle = Done(h);
        }
        public override void OnDestroy() {
            work?.Dispose(); work = null; drainageWork?.Dispose(); drainageWork = null; area?.Dispose(); area = null;
            plane?.Dispose(); plane = null; tally?.Dispose(); tally = null;
        }
    }

    public class MfdFluvialStage : PipelineStage {
        // Multiple-flow implicit stream-power erosion (new-framework feature; the model: nz_fluvial_implicit_mfd in
        // include/noize_hip.h): ImplicitFluvialStage's step taken along EVERY lower neighbour of a cell, with the weights of
        // MfdDrainageStage -- the fan the water is spread over is what erodes, where ImplicitFluvialStage with
        // FlowRouting.Multiple cuts along the one steepest receiver.  Per iteration the stage computes the multiple-flow
        // drainage of the current heights (nz_drainage_mfd, into its own plane) and solves the step
        // (nz_fluvial_implicit_mfd), both with the same exponent (1..16), the solve told to proceed by the drainage call's
        // converged word on the device; nothing is read back in between.  Pits stay pits: put DepressionFillStage in front.
        // The heights ping-pong between the payload's plane and its WRITE plane (or a plane of the stage's); the result is
        // in the payload's `data` when the handle completes.  seaLevel, rainMap / hardness / upliftMap: as
        // ImplicitFluvialStage's.  maxPasses null means the default, 128 + resolution / 2, for the drainage series and for
        // the solve each; a budget that runs out is no error: that iteration leaves the heights as they were.  Drainage is
        // the area the last iteration saw; Steps, Passes and Converged wait for the handle and read the stage's tally: the
        // iterations applied, the solve passes that did work, and Steps == iterations.
        public int iterations = 1;
        public float erodibility = 0.05f, uplift = 0.002f, dt = 1f, rain = 1f, seaLevel = -float.MaxValue;
        public int exponent = 1;
        public int? maxPasses = null;
        public DeviceTile rainMap = null, hardness = null, upliftMap = null;
        DeviceTile work;                         // nz_fluvial_implicit_mfd_work_floats floats
        DeviceTile drainageWork;                 // nz_drainage_mfd's work floats; its second int32: the solve's `proceed`
        DeviceTile area, plane, tally;           // the drainage, the heights' second plane, {steps applied, passes that did work}
        int resolution, count = 1;
        static readonly IntPtr Zeros = ZeroWords();   // what the tally is set to before a run; lives as long as the process
        static IntPtr ZeroWords() {
            IntPtr p = System.Runtime.InteropServices.Marshal.AllocHGlobal(8);
            System.Runtime.InteropServices.Marshal.WriteInt64(p, 0L);
            return p;
        }
        public MfdFluvialStage(GpuContext ctx) : base(ctx) {}
        int Cells => count * resolution * resolution;
        public DeviceTile Drainage => area;
        public int? Steps => Counted(0);
        public int? Passes => Counted(1);
        public bool? Converged => Counted(0) is int s ? s == iterations : (bool?) null;
        int? Counted(int k) {
            if (tally == null) return null;
            jobHandle.Complete();
            return BitConverter.SingleToInt32Bits(tally.ToArray()[k]);
        }
        DeviceTile Size(DeviceTile t, bool want, int n) {   // a plane of the stage: resized with the payload, gone when not wanted
            if (t != null && (!want || t.Length != n)) { t.Dispose(); t = null; }
            return want && t == null ? ctx.Alloc(n) : t;
        }
        public override void Schedule(PipelineWorkItem requirements, GpuJobHandle dependency) {
            if (requirements.data is GeneratorData g) {
                resolution = g.resolution;
                count = g is GeneratorDataBatch gb ? gb.count : 1;
            }
            CheckRequirements<GeneratorData>(requirements);
            GeneratorData d = (GeneratorData) requirements.data;
            foreach (DeviceTile m in new[] { rainMap, hardness, upliftMap })   // before any launch
                if (m != null && m.Length != Cells) throw new Exception($"MfdFluvialStage: a plane of {m.Length} floats does not fit the payload's {Cells}");
            work = Size(work, true, (int) (ulong) Native.nz_fluvial_implicit_mfd_work_floats(resolution, count));
            drainageWork = Size(drainageWork, true, (int) (ulong) Native.nz_drainage_mfd_work_floats(resolution, count));
            area = Size(area, true, Cells);
            plane = Size(plane, d.write == null, Cells);
            tally = Size(tally, true, 2);
            int budget = maxPasses ?? 128 + resolution / 2;
            NzDrainageMfdDesc drain = new NzDrainageMfdDesc {
                rain = rain, seaLevel = seaLevel, maxPasses = budget, exponent = exponent,
                rainMap = rainMap != null ? rainMap.Ptr : IntPtr.Zero };
            // the solve's `proceed`: the drainage call's converged word, the second int32 of its work planes
            NzFluvialImplicitMfdDesc solve = new NzFluvialImplicitMfdDesc {
                erodibility = erodibility, uplift = uplift, dt = dt, seaLevel = seaLevel, maxPasses = budget, exponent = exponent,
                hardness = hardness != null ? hardness.Ptr : IntPtr.Zero, upliftMap = upliftMap != null ? upliftMap.Ptr : IntPtr.Zero,
                proceed = IntPtr.Add(drainageWork.Ptr, 4), tally = tally.Ptr };
            ulong h;
            Native.Check(Native.nz_tile_upload(ctx.Handle, tally.Ptr, Zeros, (UIntPtr) 2u, dependency.id, out h), "nz_tile_upload");
            // the heights ping-pong between the payload's plane and the WRITE plane (or the stage's own)
            DeviceTile cur = d.data, other = d.write ?? plane;
            bool batch = d is GeneratorDataBatch;
            for (int i = 0; i < iterations; i++) {
                if (batch) {
                    Native.Check(Native.nz_drainage_mfd_batch(ctx.Handle, cur.Ptr, area.Ptr, drainageWork.Ptr, ref drain, resolution, count, 0, IntPtr.Zero), "nz_drainage_mfd_batch");
                    Native.Check(Native.nz_fluvial_implicit_mfd_batch(ctx.Handle, cur.Ptr, area.Ptr, other.Ptr, work.Ptr, ref solve, resolution, count, 0, out h), "nz_fluvial_implicit_mfd_batch");
                } else {
                    Native.Check(Native.nz_drainage_mfd(ctx.Handle, cur.Ptr, area.Ptr, drainageWork.Ptr, ref drain, resolution, 0, IntPtr.Zero), "nz_drainage_mfd");
                    Native.Check(Native.nz_fluvial_implicit_mfd(ctx.Handle, cur.Ptr, area.Ptr, other.Ptr, work.Ptr, ref solve, resolution, 0, out h), "nz_fluvial_implicit_mfd");
                }
                DeviceTile s = cur; cur = other; other = s;
            }
            if (d.write != null) { d.data = cur; d.write = other; }   // the pair as the run left it: `data` holds the result
            else if (cur != d.data)                                   // an odd count ended in the stage's plane
                Native.Check(Native.nz_flush_write_slice(ctx.Handle, d.data.Ptr, cur.Ptr, (UIntPtr) (uint) Cells, 0, out h), "nz_flush_write_slice");
            jobHandle = Done(h);
        }
        public override void OnDestroy() {
            work?.Dispose(); work = null; drainageWork?.Dispose(); drainageWork = null; area?.Dispose(); area = null;
            plane?.Dispose(); plane = null; tally?.Dispose(); tally = null;
        }
    }

    // Linear hillslope diffusion, dh/dt = diffusivity * laplace(h), as implicit steps of any size (new-framework feature; the
    // model: nz_hillslope_diffusion in include/noize_hip.h): backward Euler split by direction, two tridiagonal line solves
    // per step, stable and free of oscillation for every dt, the border cells held.  It rounds the knife-edge ridges and
    // one-cell gullies ImplicitFluvialStage leaves; the evolution loop is [DepressionFillStage, ImplicitFluvialStage(dt = T),
    // HillslopeDiffusionStage(dt = T)], repeated.  A direct solve: no pass budget, no verdict, nothing read back.  The stage
    // works in place on the payload's `data` (GeneratorData and GeneratorDataBatch) and owns and resizes its work planes, the
    // two coefficient tables.  The defaults are a choice, not pinned by any picture.
    public class HillslopeDiffusionStage : PipelineStage {
        public float diffusivity = 0.01f, dt = 1f;
        public int iterations = 1;
        DeviceTile work;                         // nz_hillslope_diffusion_work_floats floats
        int resolution, count = 1;
        public HillslopeDiffusionStage(GpuContext ctx) : base(ctx) {}
        public override void Schedule(PipelineWorkItem requirements, GpuJobHandle dependency) {
            if (requirements.data is GeneratorData g) {
                resolution = g.resolution;
                count = g is GeneratorDataBatch gb ? gb.count : 1;
            }
            CheckRequirements<GeneratorData>(requirements);
            GeneratorData d = (GeneratorData) requirements.data;
            int need = (int) (ulong) Native.nz_hillslope_diffusion_work_floats(resolution, count);
            if (work != null && work.Length != need) { work.Dispose(); work = null; }
            if (work == null) work = ctx.Alloc(need);
            NzHillslopeDesc desc = new NzHillslopeDesc { diffusivity = diffusivity, dt = dt, iterations = iterations };
            ulong h;
            if (d is GeneratorDataBatch)
                Native.Check(Native.nz_hillslope_diffusion_batch(ctx.Handle, d.data.Ptr, d.data.Ptr, work.Ptr, ref desc, resolution, count, dependency.id, out h), "nz_hillslope_diffusion_batch");
            else
                Native.Check(Native.nz_hillslope_diffusion(ctx.Handle, d.data.Ptr, d.data.Ptr, work.Ptr, ref desc, resolution, dependency.id, out h), "nz_hillslope_diffusion");
            jobHandle = Done(h);
        }
        public override void OnDestroy() { work?.Dispose(); work = null; }
    }

    public class ImplicitFluvialStripe {
        // The implicit stream-power solve on one row stripe of a larger grid (nz_implicit_fluvial_stripe_round / _finalise): the
        // round and the finalise that DrainageAreaStage has for the drainage area, for the solve behind it.  No pipeline stage --
        // a stripe has no payload -- so no base class: the planes and words are the caller's, and so are the exchanges and the
        // votes.  Per step on every rank: DrainageAreaStage's rounds on the current heights; then rounds of ScheduleStripe -- 1
        // row of heightRows exchanged before the round with `first`, 1 row of outRows before every later one, a vote after each
        // (nz_comm_allreduce_max_i32 on `changed`, which the next round takes as its `proceed`; IntPtr.Zero in the first) -- and
        // FinaliseStripe with the verdict "the last vote was 0"; then the two height planes swap.
        readonly GpuContext ctx;
        public float erodibility = 0.05f, uplift = 0.002f, dt = 1f, seaLevel = -3.402823466e+38f;
        public IntPtr hardnessRows = IntPtr.Zero, upliftMapRows = IntPtr.Zero;  // stripe-shaped planes, owned rows filled; Zero: off
        public ImplicitFluvialStripe(GpuContext ctx) { this.ctx = ctx; }
        // one round: at most `passes` passes over the owned rows against one frozen ghost row of h' on each side (stripeWork:
        // Native.nz_implicit_fluvial_stripe_work_floats, the same buffer in every round of a solve)
        public GpuJobHandle ScheduleStripe(IntPtr heightRows, IntPtr drainageRows, IntPtr outRows, IntPtr stripeWork, ref NzStripe st,
                                           int passes, bool first, IntPtr proceed, IntPtr changed, GpuJobHandle dependency) {
            var desc = new NzFluvialImplicitDesc { erodibility = erodibility, uplift = uplift, dt = dt, seaLevel = seaLevel, maxPasses = passes,
                                                   hardness = hardnessRows, upliftMap = upliftMapRows, proceed = IntPtr.Zero, tally = IntPtr.Zero };
            ulong h;
            Native.Check(Native.nz_implicit_fluvial_stripe_round(ctx.Handle, heightRows, drainageRows, outRows, stripeWork, ref st, ref desc, first ? 1 : 0, proceed, changed, dependency.id, out h), "nz_implicit_fluvial_stripe_round");
            return ctx.Wrap(h);
        }
        // ... and the end of the rounds: all or nothing on the owned rows by the device word `converged` -- outRows stays, or
        // takes heightRows bit for bit
        public GpuJobHandle FinaliseStripe(IntPtr heightRows, IntPtr outRows, ref NzStripe st, IntPtr converged, GpuJobHandle dependency) {
            ulong h;
            Native.Check(Native.nz_implicit_fluvial_stripe_finalise(ctx.Handle, heightRows, outRows, ref st, converged, dependency.id, out h), "nz_implicit_fluvial_stripe_finalise");
            return ctx.Wrap(h);
        }
    }

    // Implicit stream-power erosion WITH sediment deposition (new-framework feature; the model: nz_fluvial_sediment in
    // include/noize_hip.h): ImplicitFluvialStage whose solve carries the xi-q deposition term, so valleys aggrade as well as
    // cut.  Everything but the solve call is inherited: per iteration the drainage call (either routing), the proceed word,
    // the plane ping-pong, Steps / Passes / Converged and the resize logic.  deposition: G >= 0, dimensionless; 0 is
    // ImplicitFluvialStage bit for bit.  sedimentIterations: the Gauss-Seidel iterations K of every solve; the iteration
    // contracts for G up to about 1, slower as G * dt grows -- read Residual.  recordFlux: keep the sediment-flux plane Q of
    // the last applied iteration in Flux.  maxPasses is the budget of each of the 2K + 1 series of a solve, and Passes counts
    // them all.  Residual waits for the handle: max |hK - h(K-1)| of the last iteration that ran, null before the first run.
    public class SedimentFluvialStage : ImplicitFluvialStage {
        public float deposition = 0.5f;
        public int sedimentIterations = 4;
        public bool recordFlux = false;
        DeviceTile flux;                         // the flux plane, with recordFlux
        public SedimentFluvialStage(GpuContext ctx) : base(ctx) {}
        public DeviceTile Flux => flux;
        public float? Residual {
            get {
                if (work == null) return null;
                jobHandle.Complete();
                return work.Offset(0, 3).ToArray()[2];   // {passes, converged, residual}
            }
        }
        protected override int SolveWorkFloats() => (int) (ulong) Native.nz_fluvial_sediment_work_floats(resolution, count);
        protected override void EnqueueSolve(bool batch, DeviceTile cur, DeviceTile other, ref NzFluvialImplicitDesc solve, out ulong h) {
            flux = Size(flux, recordFlux, Cells);
            NzFluvialSedimentDesc desc = new NzFluvialSedimentDesc {
                erodibility = solve.erodibility, uplift = solve.uplift, dt = solve.dt, seaLevel = solve.seaLevel,
                maxPasses = solve.maxPasses, hardness = solve.hardness, upliftMap = solve.upliftMap, proceed = solve.proceed,
                tally = solve.tally, deposition = deposition, iterations = sedimentIterations,
                flux = flux != null ? flux.Ptr : IntPtr.Zero };
            if (batch) {
                Native.Check(Native.nz_fluvial_sediment_batch(ctx.Handle, cur.Ptr, area.Ptr, other.Ptr, work.Ptr, ref desc, resolution, count, 0, out h), "nz_fluvial_sediment_batch");
            } else {
                Native.Check(Native.nz_fluvial_sediment(ctx.Handle, cur.Ptr, area.Ptr, other.Ptr, work.Ptr, ref desc, resolution, 0, out h), "nz_fluvial_sediment");
            }
        }
        public override void OnDestroy() {
            flux?.Dispose(); flux = null;
            base.OnDestroy();
        }
    }

    public class MeshTileStage : PipelineStage {
        public MeshType meshType = MeshType.SquareGridHeightMap;
        public MeshTileStage(GpuContext ctx) : base(ctx) {}
        public override void Schedule(PipelineWorkItem requirements, GpuJobHandle dependency) {     // :40-46
            MeshStageData d = (MeshStageData) requirements.data;
            int count = Math.Max(1, d.count);
            int nv = (int) (ulong) Native.nz_mesh_vertex_count(d.resolution) * count, ni = (int) (ulong) Native.nz_mesh_index_count(d.resolution) * count;
            if (d.vertices == null || d.vertices.Length != nv * 12) {   // Mesh.AllocateWritableMeshData(1)
                d.vertices?.Dispose(); d.indices?.Dispose();
                d.vertices = ctx.Alloc(nv * 12);                         // 48-byte records {pos3, normal3, tangent4, uv2}
                d.indices = ctx.Alloc(ni);                               // uint32
            }
            ulong h;
            if (count > 1)
                Native.Check(Native.nz_heightmap_mesh_batch(ctx.Handle, (int) meshType, d.vertices.Ptr, d.indices.Ptr, d.resolution, d.inputResolution,
                                                            d.marginPix, d.tileHeight, d.tileSize, d.data.Ptr, count, dependency.id, out h), "nz_heightmap_mesh_batch");
            else
                Native.Check(Native.nz_heightmap_mesh(ctx.Handle, (int) meshType, d.vertices.Ptr, d.indices.Ptr, d.resolution, d.inputResolution,
                                                      d.marginPix, d.tileHeight, d.tileSize, d.data.Ptr, dependency.id, out h), "nz_heightmap_mesh");
            jobHandle = Done(h);
        }
        // OnStageComplete (:48-57): Mesh.ApplyAndDisposeWritableMeshData -> copy d.vertices / d.indices into the engine's mesh
    }

    public class ConstantStage : TmpStage {
        public ConstantOperationType operation = ConstantOperationType.MULTIPLY;
        public float value = 0.5f;
        public ConstantStage(GpuContext ctx) : base(ctx) {}
        public override void Schedule(PipelineWorkItem requirements, GpuJobHandle dependency) {
            CheckRequirements<GeneratorData>(requirements);
            GeneratorData d = (GeneratorData) requirements.data;
            Native.Check(Native.nz_constant_job(ctx.Handle, (int) operation, d.data.Ptr, tmp.Ptr, value, d.resolution, dependency.id, out ulong h), "nz_constant_job");
            jobHandle = Done(h);
        }
    }

    public class ReduceStage : TmpStage {
        public ReductionType operation = ReductionType.SUBTRACT;
        public ReduceStage(GpuContext ctx) : base(ctx) {}
        public override void Schedule(PipelineWorkItem requirements, GpuJobHandle dependency) {
            CheckRequirements<ReduceData>(requirements);
            ReduceData d = (ReduceData) requirements.data;
            Native.Check(Native.nz_reduction_job(ctx.Handle, (int) operation, d.data.Ptr, d.rightData.Ptr, tmp.Ptr, d.resolution, dependency.id, out ulong h), "nz_reduction_job");
            jobHandle = Done(h);
        }
        public override void TransformData(PipelineWorkItem inputData) {                            // ReduceStage.cs:53-62
            ReduceData d = (ReduceData) inputData.data;
            inputData.data = new GeneratorData { uuid = d.uuid, data = d.data, resolution = d.resolution, xpos = d.xpos, zpos = d.zpos };
        }
    }

    // ---- upsample / downsample (new-framework; include/noize_hip.h): resolution R -> R * factor / R / factor.  The stage owns
    //      its output plane, resized when the input size changes, and hands downstream a GeneratorData(Batch) of the new
    //      resolution whose plane it is (ReduceStage.TransformData is the model); xpos / zpos scale with the resolution ----
    public enum ResampleFilter { Nearest = 0, Bilinear = 1, CatmullRom = 2 }                        // enum nz_resample_filter

    public abstract class ResampleStage : PipelineStage {
        public int factor = 2;
        public DeviceTile output;
        DeviceTile outPositions;
        int[] outHostPositions;
        protected ResampleStage(GpuContext ctx) : base(ctx) {}
        protected abstract int OutLength(int size);
        protected abstract int OutPosition(int v);
        public override void ResizeNativeContainers(int size) {
            output?.Dispose();
            output = ctx.Alloc(OutLength(size));
        }
        public override void TransformData(PipelineWorkItem inputData) {
            GeneratorData d = (GeneratorData) inputData.data;
            int res = OutPosition(d.resolution);                                                     // a resolution scales as a position does
            if (d is GeneratorDataBatch b) {
                // rescaled on the host from the payload's host copy: no wait on the device in the scheduling path, one upload
                // per new set of positions.  A payload without a host copy is read back once
                int[] pos;
                if (b.hostPositions != null) {
                    pos = (int[]) b.hostPositions.Clone();
                } else {
                    float[] raw = b.positions.ToArray();                                             // int32 pairs, four-byte elements
                    pos = new int[raw.Length];
                    Buffer.BlockCopy(raw, 0, pos, 0, 4 * raw.Length);
                }
                for (int i = 0; i < pos.Length; i++) pos[i] = OutPosition(pos[i]);
                if (outPositions == null || outHostPositions == null || !System.Linq.Enumerable.SequenceEqual(pos, outHostPositions)) {
                    outPositions?.Dispose();
                    outPositions = ctx.Alloc(pos.Length);
                    outPositions.CopyFrom(pos);
                    outHostPositions = pos;
                }
                inputData.data = new GeneratorDataBatch { uuid = d.uuid, data = output, resolution = res, positions = outPositions, hostPositions = pos, count = b.count };
            } else {
                inputData.data = new GeneratorData { uuid = d.uuid, data = output, resolution = res, xpos = OutPosition(d.xpos), zpos = OutPosition(d.zpos) };
            }
        }
        public override void OnDestroy() { output?.Dispose(); output = null; outPositions?.Dispose(); outPositions = null; outHostPositions = null; }
    }

    public class UpsampleStage : ResampleStage {
        public ResampleFilter filter = ResampleFilter.CatmullRom;
        public DeviceTile baseData;   // optional, of the OUTPUT's size: added to the upsampled plane (detail transfer)
        public UpsampleStage(GpuContext ctx) : base(ctx) {}
        protected override int OutLength(int size) => size * factor * factor;
        protected override int OutPosition(int v) => v * factor;
        public override void Schedule(PipelineWorkItem requirements, GpuJobHandle dependency) {
            CheckRequirements<GeneratorData>(requirements);
            GeneratorData d = (GeneratorData) requirements.data;
            IntPtr b = baseData != null ? baseData.Ptr : IntPtr.Zero;
            ulong h;
            if (d is GeneratorDataBatch gb) {
                Native.Check(Native.nz_upsample_batch(ctx.Handle, d.data.Ptr, d.resolution, output.Ptr, factor, (int) filter, b, gb.count, dependency.id, out h), "nz_upsample_batch");
            } else {
                Native.Check(Native.nz_upsample(ctx.Handle, d.data.Ptr, d.resolution, output.Ptr, factor, (int) filter, b, dependency.id, out h), "nz_upsample");
            }
            jobHandle = Done(h);
        }
    }

    public class DownsampleStage : ResampleStage {
        public DownsampleStage(GpuContext ctx) : base(ctx) {}
        protected override int OutLength(int size) => size / (factor * factor);
        protected override int OutPosition(int v) => v >= 0 ? v / factor : -((-v + factor - 1) / factor);   // floor
        public override void Schedule(PipelineWorkItem requirements, GpuJobHandle dependency) {
            CheckRequirements<GeneratorData>(requirements);
            GeneratorData d = (GeneratorData) requirements.data;
            ulong h;
            if (d is GeneratorDataBatch gb) {
                Native.Check(Native.nz_downsample_batch(ctx.Handle, d.data.Ptr, d.resolution, output.Ptr, factor, gb.count, dependency.id, out h), "nz_downsample_batch");
            } else {
                Native.Check(Native.nz_downsample(ctx.Handle, d.data.Ptr, d.resolution, output.Ptr, factor, dependency.id, out h), "nz_downsample");
            }
            jobHandle = Done(h);
        }
    }

    public class CurveStage : TmpStage {
        public Func<float, float> unityCurve = t => t;   // stands in for UnityEngine.AnimationCurve.Evaluate
        public int samples = 256;
        DeviceTile curve;
        public CurveStage(GpuContext ctx) : base(ctx) {}
        public override void ResizeNativeContainers(int size) {                                      // CurveStage.cs:26-40
            base.ResizeNativeContainers(size);
            curve?.Dispose();
            curve = ctx.Alloc(samples);
            float[] host = new float[samples];
            for (int i = 0; i < samples; i++) host[i] = unityCurve((float) i / (float) samples);
            curve.CopyFrom(host);
        }
        public override void Schedule(PipelineWorkItem requirements, GpuJobHandle dependency) {
            CheckRequirements<GeneratorData>(requirements);
            GeneratorData d = (GeneratorData) requirements.data;
            Native.Check(Native.nz_curve_job(ctx.Handle, d.data.Ptr, tmp.Ptr, curve.Ptr, samples, d.resolution, dependency.id, out ulong h), "nz_curve_job");
            jobHandle = Done(h);
        }
        public override void OnDestroy() { base.OnDestroy(); curve?.Dispose(); curve = null; }
    }
}
