// noize_pipeline.hpp -- C++ host side above the C ABI: the reference's Pipeline / PipelineStage operator
// API for the hot path, for hosts written in a compiled language (the reference's own host language,
// C#, has no toolchain in this image; its P/Invoke form is in INTEGRATION.md).
//
// Same class names, field names, argument meaning and error behaviour as
//   Pipeline/Stage/PipelineStage.cs:10-62, Pipeline/Stage/StageIO.cs:8-11,
//   Pipeline/Stage/StageIOTypes/{GeneratorData,MeshStageData}.cs, Pipeline/Stage/PipelineDefinition.cs:18-25,
//   Pipeline/Executable/Pipeline.cs:19-287, Noise/NoiseStage.cs:13-61, Filter/KernelFilterStage.cs:13-51,
//   Filter/Kernel/Blur/Stage{Gaussian,Smooth}Blur.cs, Geologic/Stage/FlowMapStage.cs:16-220,
//   Mesh/Stage/MeshTileStage.cs:28-61.
// Header-only; link with -lnoize_hip.
#pragma once

#include <algorithm>
#include <array>
#include <cstdio>
#include <deque>
#include <functional>
#include <map>
#include <memory>
#include <stdexcept>
#include <string>
#include <typeinfo>
#include <vector>

#include "../../include/noize_hip.h"

namespace noize {

struct NoizeError : std::runtime_error {
    int32_t status;
    NoizeError(int32_t s, const std::string &where)
        : std::runtime_error(where + " failed with status " + std::to_string(s) + ": " + nz_last_error()), status(s) {}
};

inline void check(int32_t status, const char *where) {
    if (status != NZ_OK) throw NoizeError(status, where);
}

// Unity.Jobs.JobHandle
struct JobHandle {
    nz_ctx *ctx = nullptr;
    nz_handle id = 0;
    bool IsCompleted() const {
        if (!ctx || id == 0) return true;
        int32_t done = 0;
        check(nz_handle_query(ctx, id, &done), "nz_handle_query");
        return done != 0;
    }
    void Complete() const {
        if (ctx && id) check(nz_handle_wait(ctx, id), "nz_handle_wait");
    }
};

// NativeArray<float> / NativeSlice<float> in HBM
struct DeviceTile {
    nz_ctx *ctx = nullptr;
    float *ptr = nullptr;
    size_t Length = 0;
    bool owned = false;
    DeviceTile() = default;
    DeviceTile(nz_ctx *c, size_t n) : ctx(c), Length(n), owned(true) { check(nz_tile_alloc(c, n, &ptr), "nz_tile_alloc"); }
    DeviceTile(const DeviceTile &) = delete;
    DeviceTile &operator=(const DeviceTile &) = delete;
    ~DeviceTile() { Dispose(); }
    bool IsCreated() const { return ptr != nullptr; }
    void Dispose() {
        if (owned && ptr) nz_tile_free(ctx, ptr);
        ptr = nullptr;
    }
    void CopyFrom(const float *host) {
        check(nz_tile_upload(ctx, ptr, host, Length, 0, nullptr), "nz_tile_upload");
        check(nz_ctx_synchronize(ctx), "nz_ctx_synchronize");
    }
    void CopyTo(float *host) const {
        check(nz_tile_download(ctx, ptr, host, Length, 0, nullptr), "nz_tile_download");
        check(nz_ctx_synchronize(ctx), "nz_ctx_synchronize");
    }
};

// ---- StageIO payloads ------------------------------------------------------------------------
struct StageIO {
    std::string uuid;
    DeviceTile *data = nullptr;  // NativeSlice<float>
    virtual ~StageIO() = default;
};

struct GeneratorData : StageIO {
    int resolution = 512, xpos = 0, zpos = 0;
    // optional WRITE slice of the tile's RWTileData pair (Pipeline/Tiles/TileData.cs:49-93; new-framework): with it
    // the stencil stages run their nz_*_rw forms and TileHelpers.SWAP_RWTILE swaps `data` and `write` instead of
    // copying, so after a stage `data` is whichever of the two planes holds the result
    DeviceTile *write = nullptr;
};

struct GeneratorDataBatch;
// the payload's READ / WRITE pair as nz_rw_tile, and back (adopts the pair as the call left it)
inline nz_rw_tile rw_pair(GeneratorData *d, int count) { return nz_rw_tile{d->data->ptr, d->write->ptr, d->resolution, count}; }
inline void rw_adopt(GeneratorData *d, const nz_rw_tile &t) {
    if (t.read != d->data->ptr) std::swap(d->data, d->write);
}

// New-framework payload: `count` independent tiles of resolution^2 cells stored back to back in `data`,
// world positions {xpos, zpos} per tile in the device int32 array `positions` (see nz_*_batch).
struct GeneratorDataBatch : GeneratorData {
    int count = 1;
    const int32_t *positions = nullptr;
    std::vector<int32_t> hostPositions;  // the same pairs on the host (optional): for a stage that rescales them
};

inline int tile_count(GeneratorData *d) {
    auto *b = dynamic_cast<GeneratorDataBatch *>(d);
    return b ? b->count : 1;
}

struct MeshBuffers {  // stands in for UnityEngine.Mesh + Mesh.MeshData (PositionStream32 layout)
    std::unique_ptr<DeviceTile> vertices, indices;
    size_t vertexCount = 0, indexCount = 0;
};

struct MeshStageData : StageIO {
    int resolution = 512, inputResolution = 512, marginPix = 5;
    float tileSize = 512.f, tileHeight = 512.f;
    int xpos = 0, zpos = 0;
    MeshBuffers *mesh = nullptr;
    int count = 1;  // new-framework: `count` height planes stored back to back -> `count` meshes (nz_heightmap_mesh_batch)
};

class PipelineStateManager;

struct PipelineWorkItem {
    StageIO *data = nullptr;
    std::function<void(StageIO *)> completeAction;
    std::function<void(StageIO *, JobHandle)> scheduledAction;
    JobHandle dependency;
    PipelineStateManager *stageManager = nullptr;  // Pipeline/Stage/PipelineDefinition.cs:18-25
};

struct DownsampleData : StageIO {  // StageIOTypes/DownsampleData.cs:9-17
    int resolution = 512, inputResolution = 512;
    DeviceTile *inputData = nullptr;
};

// ---- PipelineStateManager, NativeArray<float> part (Pipeline/PipelineState/PipelineStateManager.cs:13-189,
//      PipelineState.cs:230-349) with the job-fence lock of PipelineStateLock.cs:12-27: named device buffers shared
//      between pipelines, locked while a scheduled write to them has not completed ------------------------------
class PipelineStateManager {
  public:
    explicit PipelineStateManager(nz_ctx *c) : ctx(c) {}
    DeviceTile *GetBuffer(const std::string &name, long size = -1) {
        auto it = buffers.find(name);
        if (it == buffers.end()) {
            if (size < 0) throw std::invalid_argument("No allocated buffer named " + name);
            it = buffers.emplace(name, std::unique_ptr<DeviceTile>(new DeviceTile(ctx, (size_t)size))).first;
        }
        return it->second.get();
    }
    bool BufferExists(const std::string &name) const { return buffers.count(name) != 0; }
    bool ReleaseBuffer(const std::string &name) { return buffers.erase(name) != 0; }
    bool IsLocked(const std::string &key) const {
        auto it = locks.find(key);
        return it != locks.end() && !it->second.IsCompleted();  // HandleLock.isLocked
    }
    bool TrySetLock(const std::string &key, JobHandle handle, JobHandle /*spyHandle*/) {
        if (IsLocked(key)) return false;  // a completed handle is an open lock
        locks[key] = handle;
        return true;
    }
    void OnDestroy() { buffers.clear(); }

  private:
    nz_ctx *ctx;
    std::map<std::string, std::unique_ptr<DeviceTile>> buffers;
    std::map<std::string, JobHandle> locks;
};

// ---- PipelineStage ---------------------------------------------------------------------------
class BasePipeline;
class PipelineStage {
    friend class BasePipeline;  // the one-call form of the stock stage list sets the stages' handles itself

  public:
    explicit PipelineStage(nz_ctx *c) : ctx(c) {}
    virtual ~PipelineStage() = default;
    std::vector<std::function<void(PipelineWorkItem &, JobHandle)>> OnStageScheduledAction;

    virtual void ResizeNativeContainers(size_t) {}
    virtual bool IsSchedulable(const PipelineWorkItem &) { return true; }
    virtual void Schedule(PipelineWorkItem &, JobHandle) {}
    virtual void TransformData(PipelineWorkItem &) {}
    virtual void OnStageComplete() {}
    virtual void OnDestroy() {}
    nz_ctx *Context() const { return ctx; }

    template <class T>
    T *CheckRequirements(PipelineWorkItem &requirements) {
        T *d = dynamic_cast<T *>(requirements.data);
        if (!d) throw std::runtime_error("Unhandled stageio");  // PipelineStage.cs:37
        if (d->data->Length != dataLength) {
            dataLength = d->data->Length;
            ResizeNativeContainers(dataLength);
        }
        return d;
    }
    void ReceiveHandledInput(PipelineWorkItem &requirements, JobHandle dependency) {
        Schedule(requirements, dependency);
        TransformData(requirements);
        for (auto &a : OnStageScheduledAction) a(requirements, jobHandle);
    }

  protected:
    nz_ctx *ctx;
    JobHandle jobHandle;
    size_t dataLength = 0;
    JobHandle done(nz_handle h) { return JobHandle{ctx, h}; }
};

enum class FractalNoise { Sin, Perlin, PeriodicPerlin, Simplex, RotatedSimplex, Cellular, DomainRotatedPerlin, DomainRotatedSimplex };

class NoiseStage : public PipelineStage {
  public:
    using PipelineStage::PipelineStage;
    FractalNoise noiseType = FractalNoise::Sin;
    float hurst = 0.f, startingAmplitude = 1.f, stepdown = 2.f, detuneRate = 0.f;
    int octaves = 1, noiseSize = 1000;
    void Schedule(PipelineWorkItem &requirements, JobHandle dependency) override {
        auto *d = CheckRequirements<GeneratorData>(requirements);
        nz_handle h = 0;
        if (auto *b = dynamic_cast<GeneratorDataBatch *>(d)) {
            check(nz_fractal_batch(ctx, (int)noiseType, b->data->ptr, b->resolution, b->count, b->positions, hurst,
                                   startingAmplitude, stepdown, detuneRate, octaves, noiseSize, dependency.id, &h),
                  "nz_fractal_batch");
            jobHandle = done(h);
            return;
        }
        check(nz_fractal(ctx, (int)noiseType, d->data->ptr, d->resolution, hurst, startingAmplitude, stepdown,
                         detuneRate, octaves, d->xpos, d->zpos, noiseSize, dependency.id, &h), "nz_fractal");
        jobHandle = done(h);
    }
};

// new-framework: NoiseStage with an octave shape (enum nz_fractal_shape); Fbm gives the bits of NoiseStage.  The stock-list
// fast paths compare the exact type, so a shaped stage never runs there as plain fBm.
enum class FractalShape { Fbm, Billow, Ridged };

class ShapedNoiseStage : public NoiseStage {
  public:
    using NoiseStage::NoiseStage;
    FractalShape shape = FractalShape::Ridged;
    float ridgeOffset = 1.f, ridgeGain = 2.f;
    void Schedule(PipelineWorkItem &requirements, JobHandle dependency) override {
        auto *d = CheckRequirements<GeneratorData>(requirements);
        nz_handle h = 0;
        if (auto *b = dynamic_cast<GeneratorDataBatch *>(d)) {
            check(nz_fractal_shaped_batch(ctx, (int)noiseType, b->data->ptr, b->resolution, b->count, b->positions, hurst,
                                          startingAmplitude, stepdown, detuneRate, octaves, noiseSize, (int)shape,
                                          ridgeOffset, ridgeGain, dependency.id, &h),
                  "nz_fractal_shaped_batch");
            jobHandle = done(h);
            return;
        }
        check(nz_fractal_shaped(ctx, (int)noiseType, d->data->ptr, d->resolution, hurst, startingAmplitude, stepdown,
                                detuneRate, octaves, d->xpos, d->zpos, noiseSize, (int)shape, ridgeOffset, ridgeGain,
                                dependency.id, &h),
              "nz_fractal_shaped");
        jobHandle = done(h);
    }
};

// new-framework: ShapedNoiseStage read at domain-warped coordinates (nz_fractal_warped): each cell moves by
// (2q - 1) * warpStrength cells, q a plain fBm of the same basis over warpOctaves octaves at warpScale times the noise's
// frequency.  warpStrength 0 or warpOctaves 0 gives the bits of ShapedNoiseStage.
class WarpedNoiseStage : public ShapedNoiseStage {
  public:
    explicit WarpedNoiseStage(nz_ctx *c) : ShapedNoiseStage(c) { shape = FractalShape::Fbm; }
    float warpStrength = 0.f, warpScale = 1.f;
    int warpOctaves = 4;
    void Schedule(PipelineWorkItem &requirements, JobHandle dependency) override {
        auto *d = CheckRequirements<GeneratorData>(requirements);
        nz_handle h = 0;
        if (auto *b = dynamic_cast<GeneratorDataBatch *>(d)) {
            check(nz_fractal_warped_batch(ctx, (int)noiseType, b->data->ptr, b->resolution, b->count, b->positions, hurst,
                                          startingAmplitude, stepdown, detuneRate, octaves, noiseSize, (int)shape,
                                          ridgeOffset, ridgeGain, warpStrength, warpScale, warpOctaves, dependency.id, &h),
                  "nz_fractal_warped_batch");
            jobHandle = done(h);
            return;
        }
        check(nz_fractal_warped(ctx, (int)noiseType, d->data->ptr, d->resolution, hurst, startingAmplitude, stepdown,
                                detuneRate, octaves, d->xpos, d->zpos, noiseSize, (int)shape, ridgeOffset, ridgeGain,
                                warpStrength, warpScale, warpOctaves, dependency.id, &h),
              "nz_fractal_warped");
        jobHandle = done(h);
    }
};

class TmpStage : public PipelineStage {  // stages that own one scratch plane
  public:
    using PipelineStage::PipelineStage;
    void ResizeNativeContainers(size_t) override { tmp.reset(new DeviceTile(ctx, dataLength)); }
    void OnDestroy() override { tmp.reset(); }

  protected:
    std::unique_ptr<DeviceTile> tmp;
};

class KernelFilterStage : public TmpStage {
  public:
    using TmpStage::TmpStage;
    int filter = NZ_GAUSS9_S1;
    int iterations = 1;
    void Schedule(PipelineWorkItem &requirements, JobHandle dependency) override {
        auto *d = CheckRequirements<GeneratorData>(requirements);
        nz_handle h = 0;
        if (d->write && filter != NZ_SOBEL3_2D) {
            nz_rw_tile t = rw_pair(d, tile_count(d));
            check(nz_kernel_filter_stage_rw(ctx, &t, filter, iterations, dependency.id, &h), "nz_kernel_filter_stage_rw");
            rw_adopt(d, t);
            jobHandle = done(h);
            return;
        }
        if (auto *b = dynamic_cast<GeneratorDataBatch *>(d)) {
            check(nz_kernel_filter_stage_batch(ctx, b->data->ptr, tmp->ptr, filter, iterations, b->resolution, b->count,
                                               dependency.id, &h), "nz_kernel_filter_stage_batch");
            jobHandle = done(h);
            return;
        }
        check(nz_kernel_filter_stage(ctx, d->data->ptr, tmp->ptr, filter, iterations, d->resolution, dependency.id, &h),
              "nz_kernel_filter_stage");
        jobHandle = done(h);
    }
};

inline int limitWidth(int width) {  // BlurHelper.limitWidth, Filter/Kernel/Blur/BlurKernels.cs:29-36
    if (width % 2 == 0) width += 1;
    if (width > 25) width = 25;
    return width < 3 ? 3 : width;
}

class StageGaussianBlur : public TmpStage {
  public:
    using TmpStage::TmpStage;
    int iterations = 1, sigma = 0, width = 3;
    void Schedule(PipelineWorkItem &requirements, JobHandle dependency) override {
        auto *d = CheckRequirements<GeneratorData>(requirements);
        nz_handle h = 0;
        if (d->write) {
            nz_rw_tile t = rw_pair(d, tile_count(d));
            check(nz_gauss_blur_stage_rw(ctx, &t, limitWidth(width), sigma, iterations, dependency.id, &h),
                  "nz_gauss_blur_stage_rw");
            rw_adopt(d, t);
            jobHandle = done(h);
            return;
        }
        if (auto *b = dynamic_cast<GeneratorDataBatch *>(d)) {
            check(nz_gauss_blur_stage_batch(ctx, b->data->ptr, tmp->ptr, limitWidth(width), sigma, iterations, b->resolution,
                                            b->count, dependency.id, &h), "nz_gauss_blur_stage_batch");
            jobHandle = done(h);
            return;
        }
        check(nz_gauss_blur_stage(ctx, d->data->ptr, tmp->ptr, limitWidth(width), sigma, iterations, d->resolution,
                                  dependency.id, &h), "nz_gauss_blur_stage");
        jobHandle = done(h);
    }
};

class StageSmoothBlur : public TmpStage {
  public:
    using TmpStage::TmpStage;
    int iterations = 1, width = 1;
    void Schedule(PipelineWorkItem &requirements, JobHandle dependency) override {
        auto *d = CheckRequirements<GeneratorData>(requirements);
        nz_handle h = 0;
        if (d->write && tile_count(d) == 1) {
            nz_rw_tile t = rw_pair(d, 1);
            check(nz_smooth_blur_stage_rw(ctx, &t, limitWidth(width), iterations, dependency.id, &h),
                  "nz_smooth_blur_stage_rw");
            rw_adopt(d, t);
            jobHandle = done(h);
            return;
        }
        check(nz_smooth_blur_stage(ctx, d->data->ptr, tmp->ptr, limitWidth(width), iterations, d->resolution,
                                   dependency.id, &h), "nz_smooth_blur_stage");
        jobHandle = done(h);
    }
};

class ErosionStage : public TmpStage {  // ErosionKernelJob x iterations (no stage wrapper in the reference)
  public:
    using TmpStage::TmpStage;
    int iterations = 1;
    void Schedule(PipelineWorkItem &requirements, JobHandle dependency) override {
        auto *d = CheckRequirements<GeneratorData>(requirements);
        nz_handle h = 0;
        if (d->write) {
            nz_rw_tile t = rw_pair(d, tile_count(d));
            check(nz_erosion_stage_rw(ctx, &t, iterations, dependency.id, &h), "nz_erosion_stage_rw");
            rw_adopt(d, t);
            jobHandle = done(h);
            return;
        }
        if (auto *b = dynamic_cast<GeneratorDataBatch *>(d)) {
            check(nz_erosion_stage_batch(ctx, b->data->ptr, tmp->ptr, iterations, b->resolution, b->count, dependency.id,
                                         &h), "nz_erosion_stage_batch");
            jobHandle = done(h);
            return;
        }
        check(nz_erosion_stage(ctx, d->data->ptr, tmp->ptr, iterations, d->resolution, dependency.id, &h),
              "nz_erosion_stage");
        jobHandle = done(h);
    }
};

// ---- element-wise stages (Filter/ConstantStage.cs, Filter/Reduce/ReduceStage.cs, Filter/Curve/CurveStage.cs,
//      Filter/Kernel/Blur/StageThermalErosion.cs) ---------------------------------------------------------
struct ReduceData : StageIO {  // StageIOTypes/ReduceData.cs
    int resolution = 512, xpos = 0, zpos = 0;
    DeviceTile *rightData = nullptr;
};

class ConstantStage : public TmpStage {
  public:
    using TmpStage::TmpStage;
    int operation = 0;  // ConstantOperationType {MULTIPLY, BINARIZE}
    float value = 0.5f;
    void Schedule(PipelineWorkItem &requirements, JobHandle dependency) override {
        auto *d = CheckRequirements<GeneratorData>(requirements);
        nz_handle h = 0;
        check(nz_constant_job(ctx, operation, d->data->ptr, tmp->ptr, value, d->resolution, dependency.id, &h),
              "nz_constant_job");
        jobHandle = done(h);
    }
};

class ReduceStage : public TmpStage {
  public:
    using TmpStage::TmpStage;
    int operation = 0;  // ReductionType {SUBTRACT, MULTIPLY, ROOTSUMSQUARES, MAX, MIN}
    void Schedule(PipelineWorkItem &requirements, JobHandle dependency) override {
        auto *d = CheckRequirements<ReduceData>(requirements);
        nz_handle h = 0;
        check(nz_reduction_job(ctx, operation, d->data->ptr, d->rightData->ptr, tmp->ptr, d->resolution, dependency.id, &h),
              "nz_reduction_job");
        jobHandle = done(h);
    }
    void TransformData(PipelineWorkItem &inputData) override {  // ReduceStage.cs:53-62
        auto *d = static_cast<ReduceData *>(inputData.data);
        out.uuid = d->uuid;
        out.data = d->data;
        out.resolution = d->resolution;
        out.xpos = d->xpos;
        out.zpos = d->zpos;
        inputData.data = &out;
    }

  private:
    GeneratorData out;
};

// ---- upsample / downsample (new-framework; include/noize_hip.h): resolution R -> R * factor / R / factor.  The stage owns
//      its output plane, resized when the input size changes, and hands downstream a GeneratorData(Batch) of the new
//      resolution whose plane it is (ReduceStage::TransformData is the model); xpos / zpos scale with the resolution ----
enum class ResampleFilter { Nearest, Bilinear, CatmullRom };

class ResampleStage : public PipelineStage {
  public:
    using PipelineStage::PipelineStage;
    int factor = 2;
    DeviceTile *output() { return out_tile.get(); }
    void ResizeNativeContainers(size_t n) override { out_tile.reset(new DeviceTile(ctx, out_length(n))); }
    void TransformData(PipelineWorkItem &inputData) override {
        auto *d = static_cast<GeneratorData *>(inputData.data);
        GeneratorData *o = &out;
        if (auto *b = dynamic_cast<GeneratorDataBatch *>(d)) {
            // rescaled on the host from the payload's host copy: no wait on the device in the scheduling path, one upload
            // per new set of positions.  A payload without a host copy is read back once
            std::vector<int32_t> pos = b->hostPositions;
            if (pos.size() != 2 * (size_t)b->count) {
                pos.resize(2 * (size_t)b->count);
                check(nz_tile_download(ctx, reinterpret_cast<float *>(const_cast<int32_t *>(b->positions)),
                                       reinterpret_cast<float *>(pos.data()), pos.size(), 0, nullptr), "nz_tile_download");
                check(nz_ctx_synchronize(ctx), "nz_ctx_synchronize");
            }
            for (auto &v : pos) v = out_position(v);
            if (!out_positions || pos != out_batch.hostPositions) {
                out_positions.reset(new DeviceTile(ctx, pos.size()));
                out_positions->CopyFrom(reinterpret_cast<const float *>(pos.data()));
                out_batch.hostPositions = pos;
            }
            out_batch.count = b->count;
            out_batch.positions = reinterpret_cast<const int32_t *>(out_positions->ptr);
            o = &out_batch;
        } else {
            o->xpos = out_position(d->xpos);
            o->zpos = out_position(d->zpos);
        }
        o->uuid = d->uuid;
        o->data = out_tile.get();
        o->resolution = out_position(d->resolution);  // a resolution scales as a position does
        inputData.data = o;
    }
    void OnDestroy() override {
        out_tile.reset();
        out_positions.reset();
    }

  protected:
    virtual size_t out_length(size_t n) const = 0;
    virtual int out_position(int v) const = 0;
    std::unique_ptr<DeviceTile> out_tile, out_positions;

  private:
    GeneratorData out;
    GeneratorDataBatch out_batch;
};

class UpsampleStage : public ResampleStage {
  public:
    using ResampleStage::ResampleStage;
    ResampleFilter filter = ResampleFilter::CatmullRom;
    DeviceTile *base = nullptr;  // optional, of the OUTPUT's size: added to the upsampled plane (detail transfer)
    void Schedule(PipelineWorkItem &requirements, JobHandle dependency) override {
        auto *d = CheckRequirements<GeneratorData>(requirements);
        nz_handle h = 0;
        const float *b = base ? base->ptr : nullptr;
        if (auto *gb = dynamic_cast<GeneratorDataBatch *>(d)) {
            check(nz_upsample_batch(ctx, d->data->ptr, d->resolution, out_tile->ptr, factor, (int)filter, b, gb->count,
                                    dependency.id, &h), "nz_upsample_batch");
        } else {
            check(nz_upsample(ctx, d->data->ptr, d->resolution, out_tile->ptr, factor, (int)filter, b, dependency.id, &h),
                  "nz_upsample");
        }
        jobHandle = done(h);
    }

  protected:
    size_t out_length(size_t n) const override { return n * factor * factor; }
    int out_position(int v) const override { return v * factor; }
};

class DownsampleStage : public ResampleStage {
  public:
    using ResampleStage::ResampleStage;
    void Schedule(PipelineWorkItem &requirements, JobHandle dependency) override {
        auto *d = CheckRequirements<GeneratorData>(requirements);
        nz_handle h = 0;
        if (auto *gb = dynamic_cast<GeneratorDataBatch *>(d)) {
            check(nz_downsample_batch(ctx, d->data->ptr, d->resolution, out_tile->ptr, factor, gb->count, dependency.id, &h),
                  "nz_downsample_batch");
        } else {
            check(nz_downsample(ctx, d->data->ptr, d->resolution, out_tile->ptr, factor, dependency.id, &h), "nz_downsample");
        }
        jobHandle = done(h);
    }

  protected:
    size_t out_length(size_t n) const override { return n / ((size_t)factor * factor); }
    int out_position(int v) const override { return v >= 0 ? v / factor : -((-v + factor - 1) / factor); }  // floor
};

class CurveStage : public TmpStage {
  public:
    using TmpStage::TmpStage;
    std::function<float(float)> unityCurve = [](float t) { return t; };  // AnimationCurve.Evaluate
    int samples = 256;
    void ResizeNativeContainers(size_t n) override {
        TmpStage::ResizeNativeContainers(n);
        std::vector<float> host(samples);
        for (int i = 0; i < samples; i++) host[i] = unityCurve((float)i / (float)samples);  // ExtractCurve :32-40
        curve.reset(new DeviceTile(ctx, samples));
        curve->CopyFrom(host.data());
    }
    void Schedule(PipelineWorkItem &requirements, JobHandle dependency) override {
        auto *d = CheckRequirements<GeneratorData>(requirements);
        nz_handle h = 0;
        check(nz_curve_job(ctx, d->data->ptr, tmp->ptr, curve->ptr, samples, d->resolution, dependency.id, &h),
              "nz_curve_job");
        jobHandle = done(h);
    }
    void OnDestroy() override {
        TmpStage::OnDestroy();
        curve.reset();
    }

  private:
    std::unique_ptr<DeviceTile> curve;
};

class StageThermalErosion : public PipelineStage {
  public:
    using PipelineStage::PipelineStage;
    int iterations = 1, talus = 45;
    float increment = 0.5f, meshHeightWidthRatio = 0.75f;
    void Schedule(PipelineWorkItem &requirements, JobHandle dependency) override {
        auto *d = CheckRequirements<GeneratorData>(requirements);
        nz_handle h = 0;
        check(nz_thermal_erosion(ctx, d->data->ptr, (float)talus, increment, meshHeightWidthRatio, iterations,
                                 d->resolution, dependency.id, &h), "nz_thermal_erosion");
        jobHandle = done(h);
    }
};

class FlowMapStage : public PipelineStage {
  public:
    using PipelineStage::PipelineStage;
    int iterations = 5;
    float normMin = -.1f, normMax = .1f;
    void ResizeNativeContainers(size_t) override {
        work.reset(new DeviceTile(ctx, 11 * dataLength));  // nz_flowmap_stage_work_floats per tile of the payload
    }
    void Schedule(PipelineWorkItem &requirements, JobHandle dependency) override {
        auto *g = dynamic_cast<GeneratorData *>(requirements.data);
        if (!g) throw std::runtime_error("Unhandled stageio");
        resolution = g->resolution;
        auto *d = CheckRequirements<GeneratorData>(requirements);
        nz_handle h = 0;
        if (d->write) {
            nz_rw_tile t = rw_pair(d, tile_count(d));
            check(nz_flowmap_stage_rw(ctx, &t, work->ptr, iterations, normMin, normMax, dependency.id, &h),
                  "nz_flowmap_stage_rw");
            rw_adopt(d, t);
            jobHandle = done(h);
            return;
        }
        if (auto *b = dynamic_cast<GeneratorDataBatch *>(d)) {
            check(nz_flowmap_stage_batch(ctx, b->data->ptr, work->ptr, iterations, normMin, normMax, b->resolution,
                                         b->count, dependency.id, &h), "nz_flowmap_stage_batch");
            jobHandle = done(h);
            return;
        }
        check(nz_flowmap_stage(ctx, d->data->ptr, work->ptr, iterations, normMin, normMax, d->resolution,
                               dependency.id, &h), "nz_flowmap_stage");
        jobHandle = done(h);
    }
    void OnDestroy() override { work.reset(); }

  private:
    int resolution = 0;
    std::unique_ptr<DeviceTile> work;
};

// Grid hydraulic erosion with sediment transport (new-framework feature; the model: nz_hydraulic_erosion_stage in
// include/noize_hip.h).  Owns its work planes like FlowMapStage; once the handle completes, water() holds the final water
// depth of the last payload (waterLength() floats: count * resolution^2), a river and lake mask.
// border = Open lets water and sediment run off the tile; rainMap / hardness are planes of the payload's size the caller
// supplies and keeps alive (rain * rainMap, dissolve * (1 - hardness)); recordMasks makes the stage own wear() and
// deposits(), waterLength() floats each.  With all four at their defaults the stage calls the plain entries.
enum class HydraulicBorder { Closed, Open };

class HydraulicErosionStage : public PipelineStage {
  public:
    using PipelineStage::PipelineStage;
    int iterations = 200;
    float initialWater = 1e-4f, rain = 1e-4f, evaporation = .01f, capacity = 1.f, dissolve = .3f, deposit = .3f,
          minTilt = .01f;
    HydraulicBorder border = HydraulicBorder::Closed;
    const DeviceTile *rainMap = nullptr, *hardness = nullptr;
    bool recordMasks = false;
    void ResizeNativeContainers(size_t) override {
        work.reset(new DeviceTile(ctx, nz_hydraulic_erosion_work_floats(resolution, count)));
        masks.reset(recordMasks ? new DeviceTile(ctx, 2 * waterLength()) : nullptr);
    }
    void Schedule(PipelineWorkItem &requirements, JobHandle dependency) override {
        auto *g = dynamic_cast<GeneratorData *>(requirements.data);
        if (!g) throw std::runtime_error("Unhandled stageio");
        resolution = g->resolution;
        count = tile_count(g);
        auto *d = CheckRequirements<GeneratorData>(requirements);  // sized on the payload's count * resolution^2 cells
        if (!recordMasks) masks.reset();  // switched off after a payload of this length: wear() and deposits() are empty again
        nz_handle h = 0;
        if (border != HydraulicBorder::Closed || rainMap || hardness || recordMasks) {
            for (const DeviceTile *m : {rainMap, hardness})  // before any launch
                if (m && m->Length != waterLength()) throw std::runtime_error("HydraulicErosionStage: a map does not fit the payload");
            if (recordMasks && (!masks || masks->Length != 2 * waterLength())) ResizeNativeContainers(0);
            const nz_hydraulic_desc desc{iterations, initialWater, rain, evaporation, capacity, dissolve, deposit, minTilt,
                                         (int32_t)border, rainMap ? rainMap->ptr : nullptr,
                                         hardness ? hardness->ptr : nullptr, recordMasks ? masks->ptr : nullptr,
                                         recordMasks ? masks->ptr + waterLength() : nullptr};
            if (d->write) {
                nz_rw_tile t = rw_pair(d, count);
                check(nz_hydraulic_erosion_ex_rw(ctx, &t, work->ptr, &desc, dependency.id, &h), "nz_hydraulic_erosion_ex_rw");
                rw_adopt(d, t);
            } else if (auto *b = dynamic_cast<GeneratorDataBatch *>(d)) {
                check(nz_hydraulic_erosion_ex_batch(ctx, b->data->ptr, work->ptr, &desc, b->resolution, b->count,
                                                    dependency.id, &h), "nz_hydraulic_erosion_ex_batch");
            } else {
                check(nz_hydraulic_erosion_ex(ctx, d->data->ptr, work->ptr, &desc, d->resolution, dependency.id, &h),
                      "nz_hydraulic_erosion_ex");
            }
            jobHandle = done(h);
            return;
        }
        if (d->write) {
            nz_rw_tile t = rw_pair(d, count);
            check(nz_hydraulic_erosion_stage_rw(ctx, &t, work->ptr, iterations, initialWater, rain, evaporation, capacity,
                                                dissolve, deposit, minTilt, dependency.id, &h),
                  "nz_hydraulic_erosion_stage_rw");
            rw_adopt(d, t);
            jobHandle = done(h);
            return;
        }
        if (auto *b = dynamic_cast<GeneratorDataBatch *>(d)) {
            check(nz_hydraulic_erosion_stage_batch(ctx, b->data->ptr, work->ptr, iterations, initialWater, rain,
                                                   evaporation, capacity, dissolve, deposit, minTilt, b->resolution,
                                                   b->count, dependency.id, &h),
                  "nz_hydraulic_erosion_stage_batch");
            jobHandle = done(h);
            return;
        }
        check(nz_hydraulic_erosion_stage(ctx, d->data->ptr, work->ptr, iterations, initialWater, rain, evaporation,
                                         capacity, dissolve, deposit, minTilt, d->resolution, dependency.id, &h),
              "nz_hydraulic_erosion_stage");
        jobHandle = done(h);
    }
    // The stage on one row stripe of a larger grid (nz_hydraulic_stripe): `n` iterations with this stage's scalars and border
    // in one call.  The planes -- all of the stripe's shape -- are the caller's, and so is the exchange of 3 * n ghost rows
    // before the call (nz_halo_exchange on heightIn and, unless `first`, the six stateIn planes); a NULL map or mask is an
    // option left off.
    JobHandle ScheduleStripe(const float *heightIn, float *heightOut, const float *const *stateIn, float *const *stateOut,
                             float *stripeWork, const nz_stripe &st, int n, bool first, bool last, const float *rainMapRows,
                             const float *hardnessRows, float *wearRows, float *depositRows, JobHandle dependency) {
        const nz_hydraulic_desc desc{n, initialWater, rain, evaporation, capacity, dissolve, deposit, minTilt, (int32_t)border,
                                     rainMapRows, hardnessRows, wearRows, depositRows};
        nz_handle h = 0;
        check(nz_hydraulic_stripe(ctx, heightIn, heightOut, stateIn, stateOut, stripeWork, &st, &desc, first, last,
                                  dependency.id, &h), "nz_hydraulic_stripe");
        return done(h);
    }
    const float *water() const { return work ? work->ptr : nullptr; }
    size_t waterLength() const { return (size_t)count * resolution * resolution; }
    const float *wear() const { return masks ? masks->ptr : nullptr; }  // recordMasks: waterLength() floats each
    const float *deposits() const { return masks ? masks->ptr + waterLength() : nullptr; }
    void OnDestroy() override {
        work.reset();
        masks.reset();
    }

  private:
    int resolution = 0, count = 1;
    std::unique_ptr<DeviceTile> work, masks;  // masks: wear, then deposits
};

// Stream-power fluvial erosion with drainage area (new-framework feature; the model: nz_fluvial_erosion in
// include/noize_hip.h): dendritic valleys that run from the ridges to the tile's border.  Owns its work planes like
// HydraulicErosionStage; once the handle completes, drainage() holds the drainage area of the last payload
// (drainageLength() floats: count * resolution^2), the river map.  seaLevel: cells at or below it are outlets like the
// border (-FLT_MAX: off).  rainMap / hardness / upliftMap / drainageIn are planes of the payload's size the caller supplies
// and keeps alive (rain * rainMap, erodibility * (1 - hardness), uplift * upliftMap, the drainage to start from).
class FluvialErosionStage : public PipelineStage {
  public:
    using PipelineStage::PipelineStage;
    int iterations = 200;
    float erodibility = .05f, uplift = .002f, dt = 1.f, rain = 1.f, seaLevel = -3.402823466e+38f;
    const DeviceTile *rainMap = nullptr, *hardness = nullptr, *upliftMap = nullptr, *drainageIn = nullptr;
    void ResizeNativeContainers(size_t) override {
        work.reset(new DeviceTile(ctx, nz_fluvial_erosion_work_floats(resolution, count)));
    }
    void Schedule(PipelineWorkItem &requirements, JobHandle dependency) override {
        auto *g = dynamic_cast<GeneratorData *>(requirements.data);
        if (!g) throw std::runtime_error("Unhandled stageio");
        resolution = g->resolution;
        count = tile_count(g);
        auto *d = CheckRequirements<GeneratorData>(requirements);  // sized on the payload's count * resolution^2 cells
        for (const DeviceTile *m : {rainMap, hardness, upliftMap, drainageIn})  // before any launch
            if (m && m->Length != drainageLength()) throw std::runtime_error("FluvialErosionStage: a plane does not fit the payload");
        const nz_fluvial_desc desc{iterations, erodibility, uplift, dt, rain, seaLevel,
                                   rainMap ? rainMap->ptr : nullptr, hardness ? hardness->ptr : nullptr,
                                   upliftMap ? upliftMap->ptr : nullptr, drainageIn ? drainageIn->ptr : nullptr};
        nz_handle h = 0;
        if (d->write) {
            nz_rw_tile t = rw_pair(d, count);
            check(nz_fluvial_erosion_rw(ctx, &t, work->ptr, &desc, dependency.id, &h), "nz_fluvial_erosion_rw");
            rw_adopt(d, t);
        } else if (auto *b = dynamic_cast<GeneratorDataBatch *>(d)) {
            check(nz_fluvial_erosion_batch(ctx, b->data->ptr, work->ptr, &desc, b->resolution, b->count, dependency.id, &h),
                  "nz_fluvial_erosion_batch");
        } else {
            check(nz_fluvial_erosion(ctx, d->data->ptr, work->ptr, &desc, d->resolution, dependency.id, &h),
                  "nz_fluvial_erosion");
        }
        jobHandle = done(h);
    }
    // The stage on one row stripe of a larger grid (nz_fluvial_stripe): `n` iterations with this stage's scalars in one call.
    // The planes -- all of the stripe's shape -- are the caller's, and so is the exchange of 2 * n ghost rows before the call
    // (nz_halo_exchange on heightIn and, when given, drainageInRows; the maps once, before the first call); a NULL map is
    // an option left off, a NULL drainageInRows the start state.
    JobHandle ScheduleStripe(const float *heightIn, float *heightOut, float *drainageOut, float *stripeWork,
                             const nz_stripe &st, int n, const float *drainageInRows, const float *rainMapRows,
                             const float *hardnessRows, const float *upliftMapRows, JobHandle dependency) {
        const nz_fluvial_desc desc{n, erodibility, uplift, dt, rain, seaLevel, rainMapRows, hardnessRows, upliftMapRows,
                                   drainageInRows};
        nz_handle h = 0;
        check(nz_fluvial_stripe(ctx, heightIn, heightOut, drainageOut, stripeWork, &st, &desc, dependency.id, &h),
              "nz_fluvial_stripe");
        return done(h);
    }
    const float *drainage() const { return work ? work->ptr : nullptr; }
    size_t drainageLength() const { return (size_t)count * resolution * resolution; }
    void OnDestroy() override { work.reset(); }

  private:
    int resolution = 0, count = 1;
    std::unique_ptr<DeviceTile> work;
};

// Depression filling (new-framework feature; the model: nz_fill_depressions in include/noize_hip.h): every closed hollow
// is raised to its spill level plus an epsilon gradient, so that FluvialErosionStage's river network reaches the border
// from its first iteration.  Owns its work planes like FluvialErosionStage.  With recordDepth, depth() holds the lake depth
// of the last payload (depthLength() floats; zero where nothing was filled) once the handle completes; passes() and
// converged() wait for the handle and read the status words.  seaLevel: cells at or below it are outlets like the border
// (-FLT_MAX: off).  maxPasses < 1 means the default, 64 + resolution / 4; a budget that runs out is no error: converged()
// is false, the heights are as they were and the depth is zero.
class DepressionFillStage : public PipelineStage {
  public:
    using PipelineStage::PipelineStage;
    float epsilon = 1e-4f, seaLevel = -3.402823466e+38f;
    int maxPasses = 0;  // < 1: 64 + resolution / 4
    bool recordDepth = false;
    void Schedule(PipelineWorkItem &requirements, JobHandle dependency) override {
        auto *g = dynamic_cast<GeneratorData *>(requirements.data);
        if (!g) throw std::runtime_error("Unhandled stageio");
        resolution = g->resolution;
        count = tile_count(g);
        auto *d = CheckRequirements<GeneratorData>(requirements);
        // sized on (resolution, count), not on the payload's cell count alone: the per-tile bytes depend on the number of
        // 64 x 16 tiles, so two payloads of equal length can need different sizes
        const size_t need = nz_fill_depressions_work_floats(resolution, count);
        if (!work || work->Length != need) work.reset(new DeviceTile(ctx, need));
        if (!recordDepth) lakes.reset();
        else if (!lakes || lakes->Length != depthLength()) lakes.reset(new DeviceTile(ctx, depthLength()));
        const nz_fill_desc desc{epsilon, seaLevel, maxPasses >= 1 ? maxPasses : 64 + resolution / 4,
                                lakes ? lakes->ptr : nullptr};
        nz_handle h = 0;
        if (d->write) {
            nz_rw_tile t = rw_pair(d, count);
            check(nz_fill_depressions_rw(ctx, &t, work->ptr, &desc, dependency.id, &h), "nz_fill_depressions_rw");
            rw_adopt(d, t);
        } else if (auto *b = dynamic_cast<GeneratorDataBatch *>(d)) {
            check(nz_fill_depressions_batch(ctx, b->data->ptr, work->ptr, &desc, b->resolution, b->count, dependency.id, &h),
                  "nz_fill_depressions_batch");
        } else {
            check(nz_fill_depressions(ctx, d->data->ptr, work->ptr, &desc, d->resolution, dependency.id, &h),
                  "nz_fill_depressions");
        }
        jobHandle = done(h);
    }
    // The stage on one row stripe of a larger grid, one round (nz_fill_stripe): at most `passes` passes with this stage's
    // epsilon and sea level over the owned rows, against one frozen ghost row of W on each side.  The planes and words are the
    // caller's (stripeWork: nz_fill_stripe_work_floats), and so are the exchange of one row before the call -- of heightRows
    // before the round with `first`, of wRows before every later one -- and the vote after it (nz_comm_allreduce_max_i32 on
    // `changed`, which the next round takes as its `proceed`; NULL in the first).
    JobHandle ScheduleStripe(const float *heightRows, float *wRows, float *stripeWork, const nz_stripe &st, int passes,
                             bool first, const int32_t *proceed, int32_t *changed, JobHandle dependency) {
        const nz_fill_desc desc{epsilon, seaLevel, passes, nullptr};
        nz_handle h = 0;
        check(nz_fill_stripe(ctx, heightRows, wRows, stripeWork, &st, &desc, first, proceed, changed, dependency.id, &h),
              "nz_fill_stripe");
        return done(h);
    }
    // ... and the end of the rounds (nz_fill_stripe_finalise): all or nothing on the owned rows by the device word
    // `converged`, the verdict "the last vote was 0"; depthRows may be NULL.
    JobHandle FinaliseStripe(float *heightRows, const float *wRows, float *depthRows, const nz_stripe &st,
                             const int32_t *converged, JobHandle dependency) {
        nz_handle h = 0;
        check(nz_fill_stripe_finalise(ctx, heightRows, wRows, depthRows, &st, converged, dependency.id, &h),
              "nz_fill_stripe_finalise");
        return done(h);
    }
    const float *depth() const { return lakes ? lakes->ptr : nullptr; }
    size_t depthLength() const { return (size_t)count * resolution * resolution; }
    int passes() const { return status(0); }                // -1 before the first run
    bool converged() const { return status(1) == 1; }
    void OnDestroy() override { work.reset(); lakes.reset(); }

  private:
    int status(int k) const {
        if (!work) return -1;
        jobHandle.Complete();
        int32_t words[2];
        check(nz_tile_download(ctx, work->ptr, reinterpret_cast<float *>(words), 2, 0, nullptr), "nz_tile_download");
        check(nz_ctx_synchronize(ctx), "nz_ctx_synchronize");
        return words[k];
    }
    int resolution = 0, count = 1;
    std::unique_ptr<DeviceTile> work, lakes;
};

// Drainage area (new-framework feature; the model: nz_drainage_area in include/noize_hip.h): the exact flow accumulation
// over the steepest-descent tree of the payload's heights -- the river map -- in one call.  The heights pass through
// untouched.  Once the handle completes, drainage() holds the plane of the last payload (drainageLength() floats); passes()
// and converged() wait for the handle and read the status words.  seaLevel: cells at or below it are outlets like the
// border (-FLT_MAX: off).  rainMap: a plane of the payload's size the caller supplies and keeps alive (rain * rainMap).
// maxPasses < 1 means the default, 64 + resolution / 4; a budget that runs out is no error: converged() is false and the
// drainage is the start state.  out: a caller-supplied plane of the payload's size that receives the drainage -- the plane
// FluvialErosionStage::drainageIn takes; without it the stage owns the plane.
class DrainageAreaStage : public PipelineStage {
  public:
    using PipelineStage::PipelineStage;
    float rain = 1.f, seaLevel = -3.402823466e+38f;
    int maxPasses = 0;  // < 1: 64 + resolution / 4
    const DeviceTile *rainMap = nullptr;
    DeviceTile *out = nullptr;
    void Schedule(PipelineWorkItem &requirements, JobHandle dependency) override {
        auto *g = dynamic_cast<GeneratorData *>(requirements.data);
        if (!g) throw std::runtime_error("Unhandled stageio");
        resolution = g->resolution;
        count = tile_count(g);
        auto *d = CheckRequirements<GeneratorData>(requirements);
        for (const DeviceTile *m : {rainMap, static_cast<const DeviceTile *>(out)})  // before any launch
            if (m && m->Length != drainageLength()) throw std::runtime_error("DrainageAreaStage: a plane does not fit the payload");
        // sized on (resolution, count) like DepressionFillStage's: the per-tile bytes depend on the number of 64 x 16 tiles
        const size_t need = nz_drainage_area_work_floats(resolution, count);
        if (!work || work->Length != need) work.reset(new DeviceTile(ctx, need));
        if (out) plane.reset();
        else if (!plane || plane->Length != drainageLength()) plane.reset(new DeviceTile(ctx, drainageLength()));
        const nz_drainage_desc desc{rain, seaLevel, maxPasses >= 1 ? maxPasses : 64 + resolution / 4,
                                    rainMap ? rainMap->ptr : nullptr};
        float *dst = out ? out->ptr : plane->ptr;
        nz_handle h = 0;
        if (auto *b = dynamic_cast<GeneratorDataBatch *>(d)) {
            check(nz_drainage_area_batch(ctx, b->data->ptr, dst, work->ptr, &desc, b->resolution, b->count, dependency.id, &h),
                  "nz_drainage_area_batch");
        } else {
            check(nz_drainage_area(ctx, d->data->ptr, dst, work->ptr, &desc, d->resolution, dependency.id, &h),
                  "nz_drainage_area");
        }
        jobHandle = done(h);
    }
    // The stage on one row stripe of a larger grid, one round (nz_drainage_stripe_round): at most `passes` passes with this stage's
    // rain and sea level over the owned rows, against one frozen ghost row of A on each side.  The planes and words are the
    // caller's (stripeWork: nz_drainage_stripe_work_floats; rainMapRows may be NULL), and so are the exchange before the call
    // -- 2 rows of heightRows and of rainMapRows before the round with `first`, 1 row of aRows before every later one -- and
    // the vote after it (nz_comm_allreduce_max_i32 on `changed`, which the next round takes as its `proceed`; NULL in the first).
    JobHandle ScheduleStripe(const float *heightRows, float *aRows, float *stripeWork, const float *rainMapRows,
                             const nz_stripe &st, int passes, bool first, const int32_t *proceed, int32_t *changed,
                             JobHandle dependency) {
        const nz_drainage_desc desc{rain, seaLevel, passes, rainMapRows};
        nz_handle h = 0;
        check(nz_drainage_stripe_round(ctx, heightRows, aRows, stripeWork, &st, &desc, first, proceed, changed, dependency.id, &h),
              "nz_drainage_stripe_round");
        return done(h);
    }
    // ... and the end of the rounds (nz_drainage_stripe_finalise): all or nothing on the owned rows by the device word
    // `converged`, the verdict "the last vote was 0".  aRows then serves FluvialErosionStage's stripe form as its drainageIn.
    JobHandle FinaliseStripe(float *aRows, const float *rainMapRows, const nz_stripe &st, const int32_t *converged,
                             JobHandle dependency) {
        const nz_drainage_desc desc{rain, seaLevel, 1, rainMapRows};
        nz_handle h = 0;
        check(nz_drainage_stripe_finalise(ctx, aRows, &st, &desc, converged, dependency.id, &h), "nz_drainage_stripe_finalise");
        return done(h);
    }
    const float *drainage() const { return !work ? nullptr : out ? out->ptr : plane->ptr; }  // nullptr before a payload
    size_t drainageLength() const { return (size_t)count * resolution * resolution; }
    int passes() const { return status(0); }                // -1 before the first run
    bool converged() const { return status(1) == 1; }
    size_t workLength() const { return work ? work->Length : 0; }  // the floats of the work planes the stage holds now
    void OnDestroy() override { work.reset(); plane.reset(); }

  private:
    int status(int k) const {
        if (!work) return -1;
        jobHandle.Complete();
        int32_t words[2];
        check(nz_tile_download(ctx, work->ptr, reinterpret_cast<float *>(words), 2, 0, nullptr), "nz_tile_download");
        check(nz_ctx_synchronize(ctx), "nz_ctx_synchronize");
        return words[k];
    }
    int resolution = 0, count = 1;
    std::unique_ptr<DeviceTile> work, plane;
};

// How ImplicitFluvialStage routes the drainage area: Steepest gives all of a cell's water to its steepest neighbour
// (DrainageAreaStage's rule), Multiple a slope-weighted share to every lower neighbour (MfdDrainageStage's).
enum class FlowRouting { Steepest, Multiple };

// Multiple-flow drainage (new-framework feature; the model: nz_drainage_mfd in include/noize_hip.h): the flow accumulation
// of the payload's heights with every lower neighbour taking the share (slope / steepest slope) ^ exponent of a cell's
// water, normalised -- no parallel one-cell lines on hillsides, and water spreads on fans.  In every other respect the
// stage is DrainageAreaStage: the heights pass through, drainage(), passes() and converged() describe the last payload,
// seaLevel, rainMap and out mean the same, a budget that runs out is no error and leaves the start state.  exponent: 1..16;
// 1 spreads most, larger values approach DrainageAreaStage.  maxPasses < 1 means the default, 128 + resolution / 2, twice
// DrainageAreaStage's: the flow graph's paths are longer than the tree's.  The entry has no row-stripe form.
class MfdDrainageStage : public PipelineStage {
  public:
    using PipelineStage::PipelineStage;
    float rain = 1.f, seaLevel = -3.402823466e+38f;
    int exponent = 1;
    int maxPasses = 0;  // < 1: 128 + resolution / 2
    const DeviceTile *rainMap = nullptr;
    DeviceTile *out = nullptr;
    void Schedule(PipelineWorkItem &requirements, JobHandle dependency) override {
        auto *g = dynamic_cast<GeneratorData *>(requirements.data);
        if (!g) throw std::runtime_error("Unhandled stageio");
        resolution = g->resolution;
        count = tile_count(g);
        auto *d = CheckRequirements<GeneratorData>(requirements);
        for (const DeviceTile *m : {rainMap, static_cast<const DeviceTile *>(out)})  // before any launch
            if (m && m->Length != drainageLength()) throw std::runtime_error("MfdDrainageStage: a plane does not fit the payload");
        // sized on (resolution, count) like DrainageAreaStage's: the per-tile bytes depend on the number of 64 x 16 tiles
        const size_t need = nz_drainage_mfd_work_floats(resolution, count);
        if (!work || work->Length != need) work.reset(new DeviceTile(ctx, need));
        if (out) plane.reset();
        else if (!plane || plane->Length != drainageLength()) plane.reset(new DeviceTile(ctx, drainageLength()));
        const nz_drainage_mfd_desc desc{rain, seaLevel, maxPasses >= 1 ? maxPasses : 128 + resolution / 2, exponent,
                                        rainMap ? rainMap->ptr : nullptr};
        float *dst = out ? out->ptr : plane->ptr;
        nz_handle h = 0;
        if (auto *b = dynamic_cast<GeneratorDataBatch *>(d)) {
            check(nz_drainage_mfd_batch(ctx, b->data->ptr, dst, work->ptr, &desc, b->resolution, b->count, dependency.id, &h),
                  "nz_drainage_mfd_batch");
        } else {
            check(nz_drainage_mfd(ctx, d->data->ptr, dst, work->ptr, &desc, d->resolution, dependency.id, &h), "nz_drainage_mfd");
        }
        jobHandle = done(h);
    }
    const float *drainage() const { return !work ? nullptr : out ? out->ptr : plane->ptr; }  // nullptr before a payload
    size_t drainageLength() const { return (size_t)count * resolution * resolution; }
    int passes() const { return status(0); }                // -1 before the first run
    bool converged() const { return status(1) == 1; }
    size_t workLength() const { return work ? work->Length : 0; }  // the floats of the work planes the stage holds now
    void OnDestroy() override { work.reset(); plane.reset(); }

  private:
    int status(int k) const {
        if (!work) return -1;
        jobHandle.Complete();
        int32_t words[2];
        check(nz_tile_download(ctx, work->ptr, reinterpret_cast<float *>(words), 2, 0, nullptr), "nz_tile_download");
        check(nz_ctx_synchronize(ctx), "nz_ctx_synchronize");
        return words[k];
    }
    int resolution = 0, count = 1;
    std::unique_ptr<DeviceTile> work, plane;  // work: nz_drainage_mfd_work_floats floats; its first two int32: {passes, converged}
};

// Watershed (new-framework feature; the model: nz_watershed in include/noize_hip.h): the steepest-descent tree of the
// payload's heights read upstream -- which outlet or pit every cell drains to, how far along the river it lies, and the
// tree itself.  The heights pass through untouched.  Once the handle completes, basin() holds the labels of the last
// payload (cells() int32, the index of the outlet or pit inside the cell's own tile), flowLength() the flow-path length to
// it (the member the other hosts call length; here `length` is the parameter) and receivers() one code per cell (0..7 in
// the order W E S N SW SE NW NE, 8 without a receiver); passes() and converged() wait for the handle and read the status
// words.  seaLevel: cells at or below it are outlets like the border (-FLT_MAX: off).  cellSize: the length of a straight
// move.  maxPasses < 1 means the default, 64 + resolution / 4; a budget that runs out is no error: converged() is false,
// the labels are the cells' own indices and the length is zero.  length = false: labels only.  recordReceivers: keep the
// receiver plane.
class WatershedStage : public PipelineStage {
  public:
    using PipelineStage::PipelineStage;
    float seaLevel = -3.402823466e+38f, cellSize = 1.f;
    int maxPasses = 0;  // < 1: 64 + resolution / 4
    bool length = true;
    bool recordReceivers = false;
    void Schedule(PipelineWorkItem &requirements, JobHandle dependency) override {
        auto *g = dynamic_cast<GeneratorData *>(requirements.data);
        if (!g) throw std::runtime_error("Unhandled stageio");
        resolution = g->resolution;
        count = tile_count(g);
        auto *d = CheckRequirements<GeneratorData>(requirements);
        // sized on (resolution, count) like DepressionFillStage's: the per-tile bytes depend on the number of 64 x 16 tiles
        const size_t need = nz_watershed_work_floats(resolution, count, length ? 1 : 0);
        if (!work || work->Length != need) work.reset(new DeviceTile(ctx, need));
        if (!labels || labels->Length != cells()) labels.reset(new DeviceTile(ctx, cells()));
        if (!length) lengths.reset();
        else if (!lengths || lengths->Length != cells()) lengths.reset(new DeviceTile(ctx, cells()));
        const size_t codeFloats = (cells() + 3) / 4;  // one byte per cell
        if (!recordReceivers) codes.reset();
        else if (!codes || codes->Length != codeFloats) codes.reset(new DeviceTile(ctx, codeFloats));
        const nz_watershed_desc desc{seaLevel, cellSize, maxPasses >= 1 ? maxPasses : 64 + resolution / 4};
        int32_t *b = reinterpret_cast<int32_t *>(labels->ptr);
        float *l = lengths ? lengths->ptr : nullptr;
        uint8_t *r = codes ? reinterpret_cast<uint8_t *>(codes->ptr) : nullptr;
        nz_handle h = 0;
        if (auto *bd = dynamic_cast<GeneratorDataBatch *>(d)) {
            check(nz_watershed_batch(ctx, bd->data->ptr, b, l, r, work->ptr, &desc, bd->resolution, bd->count, dependency.id, &h),
                  "nz_watershed_batch");
        } else {
            check(nz_watershed(ctx, d->data->ptr, b, l, r, work->ptr, &desc, d->resolution, dependency.id, &h), "nz_watershed");
        }
        jobHandle = done(h);
    }
    const int32_t *basin() const { return labels ? reinterpret_cast<const int32_t *>(labels->ptr) : nullptr; }  // nullptr before a payload
    const float *flowLength() const { return lengths ? lengths->ptr : nullptr; }
    const uint8_t *receivers() const { return codes ? reinterpret_cast<const uint8_t *>(codes->ptr) : nullptr; }
    size_t cells() const { return (size_t)count * resolution * resolution; }
    int passes() const { return status(0); }                // -1 before the first run
    bool converged() const { return status(1) == 1; }
    size_t workLength() const { return work ? work->Length : 0; }  // the floats of the work planes the stage holds now
    void OnDestroy() override { work.reset(); labels.reset(); lengths.reset(); codes.reset(); }

  private:
    int status(int k) const {
        if (!work) return -1;
        jobHandle.Complete();
        int32_t words[2];
        check(nz_tile_download(ctx, work->ptr, reinterpret_cast<float *>(words), 2, 0, nullptr), "nz_tile_download");
        check(nz_ctx_synchronize(ctx), "nz_ctx_synchronize");
        return words[k];
    }
    int resolution = 0, count = 1;
    std::unique_ptr<DeviceTile> work, labels, lengths, codes;
};

// Stream order (new-framework feature; the model: nz_stream_order in include/noize_hip.h): the channel cells of the
// payload's heights, their Strahler order and the unbranched reaches between heads and confluences.  The heights pass
// through untouched.  Once the handle completes, order() holds one byte per cell of the last payload (0: no channel,
// 1: a head reach, +1 where two reaches of the same order meet) and links() the cell index, inside the cell's own tile, of
// the head or confluence its reach starts at (cells() int32, -1: no channel); passes() and converged() wait for the handle
// and read the status words.  seaLevel: cells at or below it are outlets like the border (-FLT_MAX: off).  drainage: a
// device plane of the payload's size the caller supplies and keeps alive, the one DrainageAreaStage's `out` received; a
// cell is a channel cell when its drainage >= threshold; nullptr: every cell is one.  maxPasses < 1 means the default,
// 64 + resolution / 4; a budget that runs out is no error: converged() is false, order is 1 on channel cells and every
// channel cell is its own link.  recordLinks: carry the link plane.  Strahler streams, as opposed to links, are the
// caller's to derive from the two planes.
class StreamOrderStage : public PipelineStage {
  public:
    using PipelineStage::PipelineStage;
    float seaLevel = -3.402823466e+38f, threshold = 0.f;
    int maxPasses = 0;  // < 1: 64 + resolution / 4
    const DeviceTile *drainage = nullptr;
    bool recordLinks = false;
    void Schedule(PipelineWorkItem &requirements, JobHandle dependency) override {
        auto *g = dynamic_cast<GeneratorData *>(requirements.data);
        if (!g) throw std::runtime_error("Unhandled stageio");
        resolution = g->resolution;
        count = tile_count(g);
        auto *d = CheckRequirements<GeneratorData>(requirements);
        if (drainage && drainage->Length != cells())  // before any launch
            throw std::runtime_error("StreamOrderStage: drainage does not fit the payload");
        // sized on (resolution, count) like DepressionFillStage's: the per-tile bytes depend on the number of 64 x 16 tiles
        const size_t need = nz_stream_order_work_floats(resolution, count, recordLinks ? 1 : 0);
        if (!work || work->Length != need) work.reset(new DeviceTile(ctx, need));
        const size_t orderFloats = (cells() + 3) / 4;  // one byte per cell
        if (!orders || orders->Length != orderFloats) orders.reset(new DeviceTile(ctx, orderFloats));
        if (!recordLinks) linkPlane.reset();
        else if (!linkPlane || linkPlane->Length != cells()) linkPlane.reset(new DeviceTile(ctx, cells()));
        const nz_stream_order_desc desc{seaLevel, threshold, maxPasses >= 1 ? maxPasses : 64 + resolution / 4,
                                        drainage ? drainage->ptr : nullptr};
        uint8_t *o = reinterpret_cast<uint8_t *>(orders->ptr);
        int32_t *l = linkPlane ? reinterpret_cast<int32_t *>(linkPlane->ptr) : nullptr;
        nz_handle h = 0;
        if (auto *bd = dynamic_cast<GeneratorDataBatch *>(d)) {
            check(nz_stream_order_batch(ctx, bd->data->ptr, o, l, work->ptr, &desc, bd->resolution, bd->count, dependency.id, &h),
                  "nz_stream_order_batch");
        } else {
            check(nz_stream_order(ctx, d->data->ptr, o, l, work->ptr, &desc, d->resolution, dependency.id, &h), "nz_stream_order");
        }
        jobHandle = done(h);
    }
    const uint8_t *order() const { return orders ? reinterpret_cast<const uint8_t *>(orders->ptr) : nullptr; }  // nullptr before a payload
    const int32_t *links() const { return linkPlane ? reinterpret_cast<const int32_t *>(linkPlane->ptr) : nullptr; }
    size_t cells() const { return (size_t)count * resolution * resolution; }
    int passes() const { return status(0); }                // -1 before the first run
    bool converged() const { return status(1) == 1; }
    size_t workLength() const { return work ? work->Length : 0; }  // the floats of the work planes the stage holds now
    void OnDestroy() override { work.reset(); orders.reset(); linkPlane.reset(); }

  private:
    int status(int k) const {
        if (!work) return -1;
        jobHandle.Complete();
        int32_t words[2];
        check(nz_tile_download(ctx, work->ptr, reinterpret_cast<float *>(words), 2, 0, nullptr), "nz_tile_download");
        check(nz_ctx_synchronize(ctx), "nz_ctx_synchronize");
        return words[k];
    }
    int resolution = 0, count = 1;
    std::unique_ptr<DeviceTile> work, orders, linkPlane;
};

// Implicit stream-power fluvial erosion (new-framework feature; the model: nz_fluvial_implicit in include/noize_hip.h):
// FluvialErosionStage's model taken with the implicit Euler step along the receiver tree -- stable for every dt, so one
// iteration carries a time step the explicit stage needs hundreds of launches for.  Per iteration the stage computes the
// exact drainage area of the current heights (nz_drainage_area, into its own plane) and solves the step
// (nz_fluvial_implicit), told to proceed by the drainage call's converged word on the device; nothing is read back in
// between.  Pits stay pits: put DepressionFillStage in front.  The heights ping-pong between the payload's plane and its
// WRITE plane (or a plane of the stage's); the result is in the payload's `data` when the handle completes.  seaLevel:
// cells at or below it are outlets like the border (-FLT_MAX: off).  rainMap / hardness / upliftMap: device planes of the
// payload's size the caller keeps alive.  maxPasses < 1 means the default, 64 + resolution / 4, for the drainage series and
// for the solve each; a budget that runs out is no error: that iteration leaves the heights as they were.  drainage() is
// the area the last iteration saw; steps(), passes() and converged() wait for the handle and read the stage's tally: the
// iterations applied, the solve passes that did work, and steps() == iterations.  routing: FlowRouting::Multiple makes the
// drainage call of every iteration nz_drainage_mfd with flowExponent (1..16), chained through the same proceed word, its
// default budget 128 + resolution / 2; the solve still lowers each cell along its steepest receiver, only the area changes.
class ImplicitFluvialStage : public PipelineStage {
  public:
    using PipelineStage::PipelineStage;
    int iterations = 1;
    float erodibility = .05f, uplift = .002f, dt = 1.f, rain = 1.f, seaLevel = -3.402823466e+38f;
    int maxPasses = 0;  // < 1: 64 + resolution / 4
    const DeviceTile *rainMap = nullptr, *hardness = nullptr, *upliftMap = nullptr;
    FlowRouting routing = FlowRouting::Steepest;
    int flowExponent = 1;
    void Schedule(PipelineWorkItem &requirements, JobHandle dependency) override {
        auto *g = dynamic_cast<GeneratorData *>(requirements.data);
        if (!g) throw std::runtime_error("Unhandled stageio");
        resolution = g->resolution;
        count = tile_count(g);
        auto *d = CheckRequirements<GeneratorData>(requirements);
        for (const DeviceTile *m : {rainMap, hardness, upliftMap})  // before any launch
            if (m && m->Length != cells()) throw std::runtime_error("ImplicitFluvialStage: a plane does not fit the payload");
        // sized on (resolution, count) like DrainageAreaStage's: the per-tile bytes depend on the number of 64 x 16 tiles
        size(work, solveWorkFloats());
        const bool multiple = routing == FlowRouting::Multiple;
        size(drainageWork, multiple ? nz_drainage_mfd_work_floats(resolution, count) : nz_drainage_area_work_floats(resolution, count));
        size(area, cells());
        if (d->write) plane.reset();
        else size(plane, cells());
        size(tally, 2);
        const int budget = maxPasses >= 1 ? maxPasses : 64 + resolution / 4;
        const nz_drainage_desc drain{rain, seaLevel, budget, rainMap ? rainMap->ptr : nullptr};
        const nz_drainage_mfd_desc spread{rain, seaLevel, maxPasses >= 1 ? maxPasses : 128 + resolution / 2, flowExponent,
                                          rainMap ? rainMap->ptr : nullptr};
        const nz_fluvial_implicit_desc solve{erodibility, uplift, dt, seaLevel, budget, hardness ? hardness->ptr : nullptr,
                                             upliftMap ? upliftMap->ptr : nullptr,
                                             reinterpret_cast<const int32_t *>(drainageWork->ptr) + 1,
                                             reinterpret_cast<int32_t *>(tally->ptr)};
        static const int32_t zeros[2] = {0, 0};
        nz_handle h = 0;
        check(nz_tile_upload(ctx, tally->ptr, reinterpret_cast<const float *>(zeros), 2, dependency.id, &h), "nz_tile_upload");
        // the heights ping-pong between the payload's plane and the WRITE plane (or the stage's own)
        DeviceTile *cur = d->data, *other = d->write ? d->write : plane.get();
        auto *b = dynamic_cast<GeneratorDataBatch *>(d);
        for (int i = 0; i < iterations; i++) {
            if (multiple) {
                check(b ? nz_drainage_mfd_batch(ctx, cur->ptr, area->ptr, drainageWork->ptr, &spread, resolution, count, 0, nullptr)
                        : nz_drainage_mfd(ctx, cur->ptr, area->ptr, drainageWork->ptr, &spread, resolution, 0, nullptr),
                      "nz_drainage_mfd");
            } else if (b) {
                check(nz_drainage_area_batch(ctx, cur->ptr, area->ptr, drainageWork->ptr, &drain, resolution, count, 0, nullptr),
                      "nz_drainage_area_batch");
            } else {
                check(nz_drainage_area(ctx, cur->ptr, area->ptr, drainageWork->ptr, &drain, resolution, 0, nullptr),
                      "nz_drainage_area");
            }
            enqueueSolve(b != nullptr, cur->ptr, other->ptr, solve, &h);
            std::swap(cur, other);
        }
        if (d->write) {  // the pair as the run left it: `data` holds the result
            d->data = cur;
            d->write = other;
        } else if (cur != d->data) {  // an odd count ended in the stage's plane
            check(nz_flush_write_slice(ctx, d->data->ptr, cur->ptr, cells(), 0, &h), "nz_flush_write_slice");
        }
        jobHandle = done(h);
    }
    const float *drainage() const { return area ? area->ptr : nullptr; }  // nullptr before a payload
    size_t cells() const { return (size_t)count * resolution * resolution; }
    int steps() const { return counted(0); }                 // -1 before the first run
    int passes() const { return counted(1); }
    bool converged() const { return counted(0) == iterations; }
    size_t workLength() const { return work ? work->Length : 0; }  // the floats of the work planes the stage holds now
    void OnDestroy() override { work.reset(); drainageWork.reset(); area.reset(); plane.reset(); tally.reset(); }

  protected:
    // the hook of a stage that derives from this one (SedimentFluvialStage): the size of `work`, and the solve of one
    // iteration, heights cur -> other, with the desc of the run
    virtual size_t solveWorkFloats() const { return nz_fluvial_implicit_work_floats(resolution, count); }
    virtual void enqueueSolve(bool batch, const float *cur, float *other, const nz_fluvial_implicit_desc &solve, nz_handle *h) {
        if (batch) {
            check(nz_fluvial_implicit_batch(ctx, cur, area->ptr, other, work->ptr, &solve, resolution, count, 0, h),
                  "nz_fluvial_implicit_batch");
        } else {
            check(nz_fluvial_implicit(ctx, cur, area->ptr, other, work->ptr, &solve, resolution, 0, h), "nz_fluvial_implicit");
        }
    }
    void size(std::unique_ptr<DeviceTile> &t, size_t need) {
        if (!t || t->Length != need) t.reset(new DeviceTile(ctx, need));
    }
    int resolution = 0, count = 1;
    std::unique_ptr<DeviceTile> work, drainageWork, area, plane, tally;

  private:
    int counted(int k) const {
        if (!tally) return -1;
        jobHandle.Complete();
        int32_t words[2];
        check(nz_tile_download(ctx, tally->ptr, reinterpret_cast<float *>(words), 2, 0, nullptr), "nz_tile_download");
        check(nz_ctx_synchronize(ctx), "nz_ctx_synchronize");
        return words[k];
    }
};

class MfdFluvialStage : public PipelineStage {
    // Multiple-flow implicit stream-power erosion (new-framework feature; the model: nz_fluvial_implicit_mfd in
    // include/noize_hip.h): ImplicitFluvialStage's step taken along EVERY lower neighbour of a cell, with the weights of
    // MfdDrainageStage -- the fan the water is spread over is what erodes, where ImplicitFluvialStage with
    // FlowRouting::Multiple cuts along the one steepest receiver.  Per iteration the stage computes the multiple-flow
    // drainage of the current heights (nz_drainage_mfd, into its own plane) and solves the step (nz_fluvial_implicit_mfd),
    // both with the same exponent (1..16), the solve told to proceed by the drainage call's converged word on the device;
    // nothing is read back in between.  Pits stay pits: put DepressionFillStage in front.  The heights ping-pong between the
    // payload's plane and its WRITE plane (or a plane of the stage's); the result is in the payload's `data` when the handle
    // completes.  seaLevel, rainMap / hardness / upliftMap: as ImplicitFluvialStage's.  maxPasses < 1 means the default,
    // 128 + resolution / 2, for the drainage series and for the solve each; a budget that runs out is no error: that
    // iteration leaves the heights as they were.  drainage() is the area the last iteration saw; steps(), passes() and
    // converged() wait for the handle and read the stage's tally: the iterations applied, the solve passes that did work,
    // and steps() == iterations.
  public:
    using PipelineStage::PipelineStage;
    int iterations = 1;
    float erodibility = .05f, uplift = .002f, dt = 1.f, rain = 1.f, seaLevel = -3.402823466e+38f;
    int exponent = 1;
    int maxPasses = 0;  // < 1: 128 + resolution / 2
    const DeviceTile *rainMap = nullptr, *hardness = nullptr, *upliftMap = nullptr;
    void Schedule(PipelineWorkItem &requirements, JobHandle dependency) override {
        auto *g = dynamic_cast<GeneratorData *>(requirements.data);
        if (!g) throw std::runtime_error("Unhandled stageio");
        resolution = g->resolution;
        count = tile_count(g);
        auto *d = CheckRequirements<GeneratorData>(requirements);
        for (const DeviceTile *m : {rainMap, hardness, upliftMap})  // before any launch
            if (m && m->Length != cells()) throw std::runtime_error("MfdFluvialStage: a plane does not fit the payload");
        size(work, nz_fluvial_implicit_mfd_work_floats(resolution, count));
        size(drainageWork, nz_drainage_mfd_work_floats(resolution, count));
        size(area, cells());
        if (d->write) plane.reset();
        else size(plane, cells());
        size(tally, 2);
        const int budget = maxPasses >= 1 ? maxPasses : 128 + resolution / 2;
        const nz_drainage_mfd_desc drain{rain, seaLevel, budget, exponent, rainMap ? rainMap->ptr : nullptr};
        // the solve's `proceed`: the drainage call's converged word, the second int32 of its work planes
        const nz_fluvial_implicit_mfd_desc solve{erodibility, uplift, dt, seaLevel, budget, exponent,
                                                 hardness ? hardness->ptr : nullptr, upliftMap ? upliftMap->ptr : nullptr,
                                                 reinterpret_cast<const int32_t *>(drainageWork->ptr) + 1,
                                                 reinterpret_cast<int32_t *>(tally->ptr)};
        static const int32_t zeros[2] = {0, 0};
        nz_handle h = 0;
        check(nz_tile_upload(ctx, tally->ptr, reinterpret_cast<const float *>(zeros), 2, dependency.id, &h), "nz_tile_upload");
        // the heights ping-pong between the payload's plane and the WRITE plane (or the stage's own)
        DeviceTile *cur = d->data, *other = d->write ? d->write : plane.get();
        auto *b = dynamic_cast<GeneratorDataBatch *>(d);
        for (int i = 0; i < iterations; i++) {
            if (b) {
                check(nz_drainage_mfd_batch(ctx, cur->ptr, area->ptr, drainageWork->ptr, &drain, resolution, count, 0, nullptr),
                      "nz_drainage_mfd_batch");
                check(nz_fluvial_implicit_mfd_batch(ctx, cur->ptr, area->ptr, other->ptr, work->ptr, &solve, resolution, count, 0, &h),
                      "nz_fluvial_implicit_mfd_batch");
            } else {
                check(nz_drainage_mfd(ctx, cur->ptr, area->ptr, drainageWork->ptr, &drain, resolution, 0, nullptr),
                      "nz_drainage_mfd");
                check(nz_fluvial_implicit_mfd(ctx, cur->ptr, area->ptr, other->ptr, work->ptr, &solve, resolution, 0, &h),
                      "nz_fluvial_implicit_mfd");
            }
            std::swap(cur, other);
        }
        if (d->write) {  // the pair as the run left it: `data` holds the result
            d->data = cur;
            d->write = other;
        } else if (cur != d->data) {  // an odd count ended in the stage's plane
            check(nz_flush_write_slice(ctx, d->data->ptr, cur->ptr, cells(), 0, &h), "nz_flush_write_slice");
        }
        jobHandle = done(h);
    }
    const float *drainage() const { return area ? area->ptr : nullptr; }  // nullptr before a payload
    size_t cells() const { return (size_t)count * resolution * resolution; }
    int steps() const { return counted(0); }                 // -1 before the first run
    int passes() const { return counted(1); }
    bool converged() const { return counted(0) == iterations; }
    size_t workLength() const { return work ? work->Length : 0; }  // the floats of the work planes the stage holds now
    void OnDestroy() override { work.reset(); drainageWork.reset(); area.reset(); plane.reset(); tally.reset(); }

  private:
    void size(std::unique_ptr<DeviceTile> &t, size_t need) {
        if (!t || t->Length != need) t.reset(new DeviceTile(ctx, need));
    }
    int counted(int k) const {
        if (!tally) return -1;
        jobHandle.Complete();
        int32_t words[2];
        check(nz_tile_download(ctx, tally->ptr, reinterpret_cast<float *>(words), 2, 0, nullptr), "nz_tile_download");
        check(nz_ctx_synchronize(ctx), "nz_ctx_synchronize");
        return words[k];
    }
    int resolution = 0, count = 1;
    std::unique_ptr<DeviceTile> work, drainageWork, area, plane, tally;
};

// Linear hillslope diffusion, dh/dt = diffusivity * laplace(h), as implicit steps of any size (new-framework feature; the
// model: nz_hillslope_diffusion in include/noize_hip.h): backward Euler split by direction, two tridiagonal line solves per
// step, stable and free of oscillation for every dt, the border cells held.  It rounds the knife-edge ridges and one-cell
// gullies ImplicitFluvialStage leaves; the evolution loop is [DepressionFillStage, ImplicitFluvialStage(dt = T),
// HillslopeDiffusionStage(dt = T)], repeated.  A direct solve: no pass budget, no verdict, nothing read back.  The stage
// works in place on the payload's `data` (GeneratorData and GeneratorDataBatch) and owns and resizes its `work`, the two
// coefficient tables.  The defaults are a choice, not pinned by any picture.
class HillslopeDiffusionStage : public PipelineStage {
  public:
    using PipelineStage::PipelineStage;
    float diffusivity = .01f, dt = 1.f;
    int iterations = 1;
    void Schedule(PipelineWorkItem &requirements, JobHandle dependency) override {
        auto *g = dynamic_cast<GeneratorData *>(requirements.data);
        if (!g) throw std::runtime_error("Unhandled stageio");
        resolution = g->resolution;
        count = tile_count(g);
        auto *d = CheckRequirements<GeneratorData>(requirements);
        const size_t need = nz_hillslope_diffusion_work_floats(resolution, count);
        if (!work || work->Length != need) work.reset(new DeviceTile(ctx, need));
        const nz_hillslope_desc desc{diffusivity, dt, iterations};
        nz_handle h = 0;
        if (dynamic_cast<GeneratorDataBatch *>(d))
            check(nz_hillslope_diffusion_batch(ctx, d->data->ptr, d->data->ptr, work->ptr, &desc, resolution, count,
                                               dependency.id, &h), "nz_hillslope_diffusion_batch");
        else
            check(nz_hillslope_diffusion(ctx, d->data->ptr, d->data->ptr, work->ptr, &desc, resolution, dependency.id, &h),
                  "nz_hillslope_diffusion");
        jobHandle = done(h);
    }
    size_t workLength() const { return work ? work->Length : 0; }  // the floats of the work planes the stage holds now
    void OnDestroy() override { work.reset(); }

  private:
    int resolution = 0, count = 1;
    std::unique_ptr<DeviceTile> work;  // nz_hillslope_diffusion_work_floats floats
};

class ImplicitFluvialStripe {
    // The implicit stream-power solve on one row stripe of a larger grid (nz_implicit_fluvial_stripe_round / _finalise): the
    // round and the finalise that DrainageAreaStage has for the drainage area, for the solve behind it.  No pipeline stage -- a
    // stripe has no payload -- so no base class: the planes and words are the caller's, and so are the exchanges and the votes.
    // Per step on every rank: DrainageAreaStage's rounds on the current heights; then rounds of ScheduleStripe -- 1 row of
    // heightRows exchanged before the round with `first`, 1 row of outRows before every later one, a vote after each
    // (nz_comm_allreduce_max_i32 on `changed`, which the next round takes as its `proceed`; NULL in the first) -- and
    // FinaliseStripe with the verdict "the last vote was 0"; then the two height planes swap.
  public:
    explicit ImplicitFluvialStripe(nz_ctx *c) : ctx(c) {}
    float erodibility = 0.05f, uplift = 0.002f, dt = 1.f, seaLevel = -3.402823466e+38f;
    const float *hardnessRows = nullptr, *upliftMapRows = nullptr;  // stripe-shaped planes, owned rows filled; NULL: off
    // one round: at most `passes` passes over the owned rows against one frozen ghost row of h' on each side (stripeWork:
    // nz_implicit_fluvial_stripe_work_floats, the same buffer in every round of a solve)
    JobHandle ScheduleStripe(const float *heightRows, const float *drainageRows, float *outRows, float *stripeWork,
                             const nz_stripe &st, int passes, bool first, const int32_t *proceed, int32_t *changed,
                             JobHandle dependency) {
        const nz_fluvial_implicit_desc desc{erodibility, uplift, dt, seaLevel, passes, hardnessRows, upliftMapRows, nullptr, nullptr};
        nz_handle h = 0;
        check(nz_implicit_fluvial_stripe_round(ctx, heightRows, drainageRows, outRows, stripeWork, &st, &desc, first, proceed,
                                               changed, dependency.id, &h),
              "nz_implicit_fluvial_stripe_round");
        return JobHandle{ctx, h};
    }
    // ... and the end of the rounds: all or nothing on the owned rows by the device word `converged` -- outRows stays, or
    // takes heightRows bit for bit
    JobHandle FinaliseStripe(const float *heightRows, float *outRows, const nz_stripe &st, const int32_t *converged,
                             JobHandle dependency) {
        nz_handle h = 0;
        check(nz_implicit_fluvial_stripe_finalise(ctx, heightRows, outRows, &st, converged, dependency.id, &h),
              "nz_implicit_fluvial_stripe_finalise");
        return JobHandle{ctx, h};
    }

  private:
    nz_ctx *ctx;
};

// Implicit stream-power erosion WITH sediment deposition (new-framework feature; the model: nz_fluvial_sediment in
// include/noize_hip.h): ImplicitFluvialStage whose solve carries the xi-q deposition term, so valleys aggrade as well as
// cut.  Everything but the solve call is inherited: per iteration the drainage call (either routing), the proceed word, the
// plane ping-pong, steps() / passes() / converged() and the resize logic.  deposition: G >= 0, dimensionless; 0 is
// ImplicitFluvialStage bit for bit.  sedimentIterations: the Gauss-Seidel iterations K of every solve; the iteration
// contracts for G up to about 1, slower as G * dt grows -- read residual().  recordFlux: keep the sediment-flux plane Q of the
// last applied iteration in flux().  maxPasses is the budget of each of the 2K + 1 series of a solve, and passes() counts
// them all.  residual() waits for the handle: max |hK - h(K-1)| of the last iteration that ran, -1 before the first run.
class SedimentFluvialStage : public ImplicitFluvialStage {
  public:
    using ImplicitFluvialStage::ImplicitFluvialStage;
    float deposition = .5f;
    int sedimentIterations = 4;
    bool recordFlux = false;
    const float *flux() const { return fluxPlane ? fluxPlane->ptr : nullptr; }  // nullptr without recordFlux
    float residual() const {
        if (!work) return -1.f;
        jobHandle.Complete();
        float words[3];
        check(nz_tile_download(ctx, work->ptr, words, 3, 0, nullptr), "nz_tile_download");
        check(nz_ctx_synchronize(ctx), "nz_ctx_synchronize");
        return words[2];
    }
    void OnDestroy() override {
        fluxPlane.reset();
        ImplicitFluvialStage::OnDestroy();
    }

  protected:
    size_t solveWorkFloats() const override { return nz_fluvial_sediment_work_floats(resolution, count); }
    void enqueueSolve(bool batch, const float *cur, float *other, const nz_fluvial_implicit_desc &solve, nz_handle *h) override {
        if (recordFlux) size(fluxPlane, cells());
        else fluxPlane.reset();
        const nz_fluvial_sediment_desc desc{solve.erodibility, solve.uplift, solve.dt, solve.seaLevel, solve.maxPasses,
                                            solve.hardness, solve.upliftMap, solve.proceed, solve.tally, deposition,
                                            sedimentIterations, fluxPlane ? fluxPlane->ptr : nullptr};
        if (batch) {
            check(nz_fluvial_sediment_batch(ctx, cur, area->ptr, other, work->ptr, &desc, resolution, count, 0, h),
                  "nz_fluvial_sediment_batch");
        } else {
            check(nz_fluvial_sediment(ctx, cur, area->ptr, other, work->ptr, &desc, resolution, 0, h), "nz_fluvial_sediment");
        }
    }

  private:
    std::unique_ptr<DeviceTile> fluxPlane;
};

class MeshTileStage : public PipelineStage {
  public:
    using PipelineStage::PipelineStage;
    int meshType = NZ_MESH_SQUARE_GRID;
    void Schedule(PipelineWorkItem &requirements, JobHandle dependency) override {
        auto *d = dynamic_cast<MeshStageData *>(requirements.data);
        if (!d || !d->mesh) throw std::runtime_error("Unhandled stageio");
        MeshBuffers &m = *d->mesh;
        size_t nv = nz_mesh_vertex_count(d->resolution) * d->count, ni = nz_mesh_index_count(d->resolution) * d->count;
        if (m.vertexCount != nv) {  // Mesh.AllocateWritableMeshData(1)
            m.vertices.reset(new DeviceTile(ctx, nv * 12));
            m.indices.reset(new DeviceTile(ctx, ni));
            m.vertexCount = nv;
            m.indexCount = ni;
        }
        nz_handle h = 0;
        if (d->count > 1) {
            check(nz_heightmap_mesh_batch(ctx, meshType, m.vertices->ptr, reinterpret_cast<uint32_t *>(m.indices->ptr),
                                          d->resolution, d->inputResolution, d->marginPix, d->tileHeight, d->tileSize,
                                          d->data->ptr, d->count, dependency.id, &h), "nz_heightmap_mesh_batch");
            jobHandle = done(h);
            return;
        }
        check(nz_heightmap_mesh(ctx, meshType, m.vertices->ptr, reinterpret_cast<uint32_t *>(m.indices->ptr),
                                d->resolution, d->inputResolution, d->marginPix, d->tileHeight, d->tileSize,
                                d->data->ptr, dependency.id, &h), "nz_heightmap_mesh");
        jobHandle = done(h);
    }
};

// ---- CropStage (Filter/Sample/CropStage.cs:11-19; the job's offset stays 0 as in CropJob.cs:43-59) -----------
class CropStage : public PipelineStage {
  public:
    using PipelineStage::PipelineStage;
    void Schedule(PipelineWorkItem &requirements, JobHandle dependency) override {
        auto *d = dynamic_cast<DownsampleData *>(requirements.data);
        if (!d) throw std::runtime_error("Unhandled stageio");
        nz_handle h = 0;
        check(nz_crop_job(ctx, d->inputData->ptr, d->inputResolution, d->data->ptr, d->resolution, dependency.id, &h),
              "nz_crop_job");
        jobHandle = done(h);
    }
};

// ---- context stages (Pipeline/PipelineState/Stage/*.cs, Mesh/Stage/MeshTileReferenceDataStage.cs) -----------
inline std::string contextBufferName(int xpos, int zpos, int resolution, const std::string &alias) {
    return std::to_string(xpos) + "_" + std::to_string(zpos) + "__" + std::to_string(resolution) + "__" + alias;
}

class ReadGeneratorContextStage : public PipelineStage {  // ReadGeneratorContextStage.cs:13-46
  public:
    using PipelineStage::PipelineStage;
    std::string contextAlias;
    bool IsSchedulable(const PipelineWorkItem &job) override {
        auto *gd = dynamic_cast<GeneratorData *>(job.data);
        if (!job.stageManager || !gd) return false;
        std::string name = contextBufferName(gd->xpos, gd->zpos, gd->resolution, contextAlias);
        return job.stageManager->BufferExists(name) && !job.stageManager->IsLocked(name);
    }
    void Schedule(PipelineWorkItem &requirements, JobHandle dependency) override {
        auto *gd = CheckRequirements<GeneratorData>(requirements);
        size_t res = (size_t)gd->resolution * gd->resolution;
        DeviceTile *buffer = requirements.stageManager->GetBuffer(
            contextBufferName(gd->xpos, gd->zpos, gd->resolution, contextAlias), (long)res);
        nz_handle h = 0;
        check(nz_flush_write_slice(ctx, gd->data->ptr, buffer->ptr, res, dependency.id, &h), "nz_flush_write_slice");
        jobHandle = done(h);
    }
};

class WriteGeneratorContextStage : public PipelineStage {  // WriteGeneratorContextStage.cs:13-46
  public:
    using PipelineStage::PipelineStage;
    std::string contextAlias;
    bool IsSchedulable(const PipelineWorkItem &job) override {
        auto *gd = dynamic_cast<GeneratorData *>(job.data);
        if (!job.stageManager || !gd) return false;
        return !job.stageManager->IsLocked(contextBufferName(gd->xpos, gd->zpos, gd->resolution, contextAlias));
    }
    void Schedule(PipelineWorkItem &requirements, JobHandle dependency) override {
        auto *gd = CheckRequirements<GeneratorData>(requirements);
        size_t res = (size_t)gd->resolution * gd->resolution;
        std::string name = contextBufferName(gd->xpos, gd->zpos, gd->resolution, contextAlias);
        DeviceTile *buffer = requirements.stageManager->GetBuffer(name, (long)res);
        nz_handle h1 = 0, h2 = 0;
        check(nz_flush_write_slice(ctx, buffer->ptr, gd->data->ptr, res, dependency.id, &h1), "nz_flush_write_slice");
        check(nz_handle_record(ctx, &h2), "nz_handle_record");  // LockJob: a no-op marker after the copy
        jobHandle = done(h2);
        requirements.stageManager->TrySetLock(name, done(h1), jobHandle);
    }
};

class MeshTileReferenceDataStage : public MeshTileStage {  // Mesh/Stage/MeshTileReferenceDataStage.cs:22-84
  public:
    using MeshTileStage::MeshTileStage;
    std::string contextAlias;
    bool IsSchedulable(const PipelineWorkItem &job) override {
        auto *d = dynamic_cast<MeshStageData *>(job.data);
        if (!job.stageManager || !d) return false;
        std::string name = contextBufferName(d->xpos, d->zpos, d->inputResolution, contextAlias);
        return job.stageManager->BufferExists(name) && !job.stageManager->IsLocked(name);
    }
    void Schedule(PipelineWorkItem &requirements, JobHandle dependency) override {
        auto *d = dynamic_cast<MeshStageData *>(requirements.data);
        if (!d) throw std::runtime_error("Unhandled stageio");
        DeviceTile *own = d->data;
        d->data = requirements.stageManager->GetBuffer(contextBufferName(d->xpos, d->zpos, d->inputResolution, contextAlias),
                                                       (long)d->inputResolution * d->inputResolution);
        try {
            MeshTileStage::Schedule(requirements, dependency);  // the mesh job reads the context buffer (:62-64)
        } catch (...) {
            d->data = own;
            throw;
        }
        d->data = own;
    }
};

// ---- BasePipeline (Pipeline/Executable/Pipeline.cs) --------------------------------------------
class BasePipeline {
  public:
    std::string alias = "Unnamed Pipeline";
    PipelineStateManager *contextManager = nullptr;  // handed to every work item (Pipeline.cs:76-104)
    explicit BasePipeline(std::vector<PipelineStage *> stages) : stage_instances(std::move(stages)) { Setup(); }
    virtual ~BasePipeline() = default;
    virtual std::vector<BasePipeline *> GetDependencies() { return {this}; }  // Pipeline.cs:63-65
    bool Idle() const { return queue.empty() && dependencyHell.empty() && !pipelineRunning && !pipelineBeingScheduled; }
    size_t Parked() const { return dependencyHell.size(); }

    void Enqueue(StageIO *input, std::function<void(StageIO *, JobHandle)> scheduleAction = nullptr,
                 std::function<void(StageIO *)> completeAction = nullptr, JobHandle dependency = JobHandle()) {
        queue.push_back(PipelineWorkItem{input, completeAction, scheduleAction, dependency, contextManager});
    }
    void Schedule(PipelineWorkItem wi) {
        activeItem = std::move(wi);
        if (stage_instances.empty()) throw std::runtime_error("No stages in pipeline");
        pipelineBeingScheduled = true;
        stage_instances[0]->ReceiveHandledInput(activeItem, activeItem.dependency);
    }
    bool WorkIsSchedulable(const PipelineWorkItem &item) {  // Pipeline.cs:256-265
        bool ready = true;
        for (auto *s : stage_instances) ready = s->IsSchedulable(item) && ready;
        return ready;
    }
    bool GetNextJob(PipelineWorkItem &out) {  // Pipeline.cs:183-214: parked items first, then the queue
        for (size_t i = 0; i < dependencyHell.size(); i++)
            if (WorkIsSchedulable(dependencyHell[i])) {
                out = dependencyHell[i];
                dependencyHell.erase(dependencyHell.begin() + i);
                return true;
            }
        while (!queue.empty()) {
            PipelineWorkItem wi = queue.front();
            queue.pop_front();
            if (WorkIsSchedulable(wi)) {
                out = wi;
                return true;
            }
            dependencyHell.push_back(wi);
        }
        return false;
    }
    virtual void Update() {
        if (!pipelineRunning && !pipelineBeingScheduled) {
            PipelineWorkItem wi;
            if (GetNextJob(wi)) Schedule(wi);
        }
    }
    // Nobody outside this pipeline has been handed a handle of the pass that is running: the work item carries no
    // scheduledAction and no stage has a scheduled-action hook beyond its hand-over to the next stage (a joint, a downstream
    // pipeline).  Work scheduled on such a handle has consumed the failed pass's planes and cannot be recalled from here.
    bool RetryIsLocal() const {
        if (activeItem.scheduledAction) return false;
        for (size_t i = 0; i < stage_instances.size(); i++)
            if (stage_instances[i]->OnStageScheduledAction.size() != 1) return false;  // (Setup() gave every stage exactly one)
        return true;
    }
    // pipelineHandle.Complete().  NZ_ERR_RETRY -- a chained kernel-filter launch timed out, the planes computed since are
    // invalid and the context has switched to separate launches -- is answered once by running the work item again, when
    // the pipeline regenerates its tile from scratch (its first stage is the NoiseStage) and the failed pass is this
    // pipeline's own business (RetryIsLocal).  The failed pass is wound up first (OnStageComplete, as after any pass); the
    // item's dependency was satisfied by the first pass and is not applied again.  Otherwise the error goes to the caller.
    void CompleteActive() {
        try {
            pipelineHandle.Complete();
        } catch (const NoizeError &e) {
            if (e.status != NZ_ERR_RETRY || !RegeneratesItsTile() || !RetryIsLocal()) throw;
            for (auto *s : stage_instances) s->OnStageComplete();
            pipelineRunning = false;
            activeItem.dependency = JobHandle();
            Schedule(activeItem);
            pipelineHandle.Complete();  // (a second failure is the caller's)
        }
    }
    bool LateUpdate() {
        if (pipelineRunning && pipelineHandle.IsCompleted()) {
            CompleteActive();
            for (auto *s : stage_instances) s->OnStageComplete();
            if (activeItem.completeAction) activeItem.completeAction(activeItem.data);
            pipelineRunning = false;
            return true;
        }
        return false;
    }
    void RunToCompletion() {  // until the queue is drained or only unschedulable items are left
        while (!queue.empty() || !dependencyHell.empty() || pipelineRunning) {
            Update();
            if (pipelineRunning) {
                CompleteActive();
                LateUpdate();
            } else if (queue.empty()) {
                break;  // everything left is parked on a dependency another pipeline has to satisfy
            }
        }
    }
    virtual void Destroy() {
        for (auto *s : stage_instances) s->OnDestroy();
    }

  protected:
    bool RegeneratesItsTile() const;  // the first stage is the NoiseStage
    void Setup() {
        PipelineStage *previous = nullptr;
        for (auto *stage : stage_instances) {
            if (previous)
                previous->OnStageScheduledAction.push_back(
                    [stage](PipelineWorkItem &wi, JobHandle h) { stage->ReceiveHandledInput(wi, h); });
            previous = stage;
        }
        if (previous)
            previous->OnStageScheduledAction.push_back([this](PipelineWorkItem &wi, JobHandle h) {
                pipelineHandle = h;
                pipelineRunning = true;
                pipelineBeingScheduled = false;
                if (activeItem.scheduledAction) activeItem.scheduledAction(wi.data, h);
            });
    }
    std::vector<PipelineStage *> stage_instances;
    std::deque<PipelineWorkItem> queue;
    std::vector<PipelineWorkItem> dependencyHell;
    PipelineWorkItem activeItem;
    JobHandle pipelineHandle;
    bool pipelineBeingScheduled = false, pipelineRunning = false;
};

// ---- ReducePipeline (Pipeline/Executable/ReducePipeline.cs:31-166) ------------------------------
// One work item -> the same tile requested from both upstream pipelines (the right one into a plane this
// pipeline owns) -> this pipeline's stages on a ReduceData of the two planes.
class ReducePipeline : public BasePipeline {
  public:
    ReducePipeline(nz_ctx *ctx, std::vector<PipelineStage *> stages, BasePipeline *left, BasePipeline *right)
        : BasePipeline(std::move(stages)), ctx(ctx), upstreamPipelineLeft(left), upstreamPipelineRight(right) {}

    std::vector<BasePipeline *> GetDependencies() override {  // :52-62
        std::vector<BasePipeline *> up{upstreamPipelineLeft, upstreamPipelineRight, this};
        for (auto *p : upstreamPipelineLeft->GetDependencies()) up.push_back(p);
        for (auto *p : upstreamPipelineRight->GetDependencies()) up.push_back(p);
        return up;
    }
    void Update() override {  // OnUpdate :64-80
        if (!pipelineRunning && !pipelineBeingScheduled && !upstreamsRunning && !queue.empty()) {
            PipelineWorkItem wi = queue.front();
            queue.pop_front();
            upstreamsRunning = true;
            ScheduleUpstreams(wi);
        }
    }
    void RunToCompletion() {  // the frame loop over this pipeline and everything upstream of it
        std::vector<BasePipeline *> pipes;
        for (auto *p : GetDependencies())
            if (std::find(pipes.begin(), pipes.end(), p) == pipes.end()) pipes.push_back(p);
        bool busy = true;
        while (busy) {
            for (auto *p : pipes) p->Update();
            for (auto *p : pipes) p->LateUpdate();
            busy = upstreamsRunning;
            for (auto *p : pipes) busy = busy || !p->Idle();
        }
    }
    void Destroy() override {  // :157-163
        rightData.reset();
        BasePipeline::Destroy();
    }

  private:
    void ScheduleUpstreams(const PipelineWorkItem &wi) {  // :82-121
        auto *leftData = dynamic_cast<GeneratorData *>(wi.data);
        if (!leftData) throw std::runtime_error("Unhandled stageio");
        if (!rightData || rightData->Length != leftData->data->Length)
            rightData.reset(new DeviceTile(ctx, leftData->data->Length));
        left = leftData;
        rightIO = *leftData;
        rightIO.data = rightData.get();
        doneLeft = doneRight = false;
        action = wi.completeAction;
        upstreamPipelineLeft->Enqueue(left, nullptr, [this](StageIO *res) { OnCompleteUpstream(res, true); });
        upstreamPipelineRight->Enqueue(&rightIO, nullptr, [this](StageIO *res) { OnCompleteUpstream(res, false); });
    }
    void OnCompleteUpstream(StageIO *res, bool isLeft) {  // :123-149
        (isLeft ? doneLeft : doneRight) = true;
        if (!(doneLeft && doneRight)) return;
        upstreamsRunning = false;
        auto *d = static_cast<GeneratorData *>(res);
        joined.uuid = d->uuid;
        joined.resolution = d->resolution;
        joined.data = left->data;
        joined.rightData = rightIO.data;
        joined.xpos = d->xpos;
        joined.zpos = d->zpos;
        Schedule(PipelineWorkItem{&joined, action, nullptr, JobHandle(), contextManager});
    }
    nz_ctx *ctx;
    BasePipeline *upstreamPipelineLeft, *upstreamPipelineRight;
    bool upstreamsRunning = false, doneLeft = false, doneRight = false;
    std::unique_ptr<DeviceTile> rightData;
    GeneratorData *left = nullptr;
    GeneratorData rightIO;
    ReduceData joined;
    std::function<void(StageIO *)> action;
};

// ---- live erosion (BASELINE config 4): Component/LiveErosion.cs:200-436 without the MonoBehaviour ----------------
enum class ErosionMode { ALL_EROSION, ONLY_THERMAL_EROSION, THERMAL_FLOW_WATER, ONLY_FLOW_WATER };  // LiveErosionDataTypes.cs:28-33

struct ErosionSettings {  // ScriptableObject/ErosionSettings.cs:5-124 (defaults = Reset())
    int CYCLES = 3, PARTICLES_PER_CYCLE = 1000;
    ErosionMode BEHAVIOR = ErosionMode::ALL_EROSION;
    float INERTIA = 0.5f, GRAVITY = 1.0f, DRAG = 0.001f, FRICTION = 0.01f, EVAP = 0.01f, EROSION = 1.0f, DEPOSITION = 0.1f;
    float FLOW_HEIGHT_CONTRIBUTION = 25.0f, SLOW_CULL_ANGLE = 3.0f, SLOW_CULL_SPEED = 0.11f, CAPACITY = 3.0f;
    int MAXAGE = 100, WATER_STEPS = 10;
    float SURFACE_EVAPORATION_RATE = 0.1f, POOL_PLACEMENT_MULTIPLIER = 0.5f, TRACK_PLACEMENT_MULTIPLIER = 80.0f,
          FLOW_LOSS_RATE = 0.05f;
    int PILING_RADIUS = 15;
    float MIN_PILE_INCREMENT = 1.0f, PILE_THRESHOLD = 2.0f;
    bool ENABLE_THERMAL = true;
    float TALUS = 55.0f, THERMAL_STEP = 0.6f;
    int THERMAL_CYCLES = 1;

    nz_erosion_params AsParameters() const {  // :96-123
        nz_erosion_params ep{};
        ep.INERTIA = INERTIA; ep.GRAVITY = GRAVITY; ep.DRAG = DRAG; ep.FRICTION = FRICTION; ep.EVAP = EVAP;
        ep.EROSION = EROSION; ep.DEPOSITION = DEPOSITION; ep.FLOW_HEIGHT_CONTRIBUTION = FLOW_HEIGHT_CONTRIBUTION;
        ep.SLOW_CULL_ANGLE = SLOW_CULL_ANGLE; ep.SLOW_CULL_SPEED = SLOW_CULL_SPEED;
        ep.CAPACITY = BEHAVIOR == ErosionMode::ALL_EROSION ? CAPACITY : 0.0f;
        ep.MAXAGE = MAXAGE;
        ep.TERMINAL_VELOCITY = 1.0f / DRAG;
        ep.SURFACE_EVAPORATION_RATE = SURFACE_EVAPORATION_RATE;
        ep.POOL_PLACEMENT_MULTIPLIER = BEHAVIOR == ErosionMode::ONLY_THERMAL_EROSION ? 0.0f : POOL_PLACEMENT_MULTIPLIER;
        ep.TRACK_PLACEMENT_MULTIPLIER = TRACK_PLACEMENT_MULTIPLIER; ep.FLOW_LOSS_RATE = FLOW_LOSS_RATE;
        ep.PILING_RADIUS = PILING_RADIUS; ep.MIN_PILE_INCREMENT = MIN_PILE_INCREMENT; ep.PILE_THRESHOLD = PILE_THRESHOLD;
        return ep;
    }
};

// Owns poolMap / streamMap / particleTrack (planes indexed x * res + z), the particle queue and the erosive events, and
// chains one Update's worth of jobs on the context's stream.  `seeds`: one per cycle (the reference draws them from
// UnityEngine.Random, MultiThreadErosionJob.cs:50): the same seeds give the same planes on every run.
class LiveErosion {
  public:
    LiveErosion(nz_ctx *c, DeviceTile *height, const nz_tile_set_meta &tm, const ErosionSettings &es, bool perform = true)
        : ctx(c), heightMap(height), tileMeta(tm), erosionSettings(es), performErosion(perform), res(tm.GENERATOR_RES[0]),
          poolMap(c, (size_t)tm.GENERATOR_RES[0] * tm.GENERATOR_RES[0]), streamMap(c, poolMap.Length),
          particleTrack(c, poolMap.Length) {
        if (height->Length != poolMap.Length) throw std::runtime_error("heightMap is not GENERATOR_RES^2 cells");
        std::vector<float> zeros(poolMap.Length, 0.0f);
        poolMap.CopyFrom(zeros.data());
        streamMap.CopyFrom(zeros.data());
        particleTrack.CopyFrom(zeros.data());
        QUEUE_SIZE = perform ? es.PARTICLES_PER_CYCLE : 1;  // :215-219
        const int n = res * res;
        check(nz_particle_queue_create(ctx, std::max(std::max(4 * QUEUE_SIZE, QUEUE_SIZE + n / 8), 1024), &particleQueue),
              "nz_particle_queue_create");
        check(nz_erosive_events_create(ctx, res, &events), "nz_erosive_events_create");
    }
    LiveErosion(const LiveErosion &) = delete;
    // nz_ctx_set_pile_safe: ErodeHeightMaps keeps a copy of the height plane, waits for the pile solver's one-launch form and runs
    // itself again colour by colour should a block of it ever give up (a property of the context)
    void SetSafe(bool on) { check(nz_ctx_set_pile_safe(ctx, on ? 1 : 0), "nz_ctx_set_pile_safe"); }
    int PileRetries() const { return nz_ctx_pile_retries(ctx); }
    ~LiveErosion() {
        jobHandle.Complete();
        if (particleQueue) nz_particle_queue_destroy(ctx, particleQueue);
        if (events) nz_erosive_events_destroy(ctx, events);
    }

    JobHandle TriggerQueuedBeyerMT(const std::vector<int> &seeds) {  // :378-436
        const ErosionSettings &es = erosionSettings;
        const nz_erosion_params ep = es.AsParameters();
        const nz_tile_set_meta &tm = tileMeta;
        nz_handle h = 0;
        // The jobs of a cycle are links of ONE chain on the context's stream: with fewHandles only the handles somebody waits
        // for are asked of the library (out = NULL otherwise) -- a handle is an event record, ~3 us of the stream
        const bool all = !fewHandles;
        auto link = [&](bool wanted) -> nz_handle * { return wanted || all ? &h : (h = 0, (nz_handle *)nullptr); };
        if (performErosion) {
            if ((int)seeds.size() < es.CYCLES) throw std::runtime_error("one seed per cycle");
            for (int i = 0; i < es.CYCLES; i++) {
                const bool last = i + 1 == es.CYCLES;  // the chain's last handle is the component's jobHandle
                nz_handle dep = h;
                if (es.ENABLE_THERMAL && es.BEHAVIOR != ErosionMode::ONLY_FLOW_WATER) {  // `TILE_SIZE.x / HEIGHT`: int / int (:386)
                    check(nz_thermal_erosion(ctx, heightMap->ptr, es.TALUS, es.THERMAL_STEP, (float)(tm.TILE_SIZE[0] / tm.HEIGHT),
                                             es.THERMAL_CYCLES, res, dep, link(false)), "nz_thermal_erosion");
                    dep = h;
                }
                if (es.BEHAVIOR != ErosionMode::ONLY_FLOW_WATER) {
                    check(nz_fill_beyer_queue(ctx, particleQueue, &ep, &tm, particleGenerationID % 4, res, QUEUE_SIZE, seeds[i],
                                              std::min(10, QUEUE_SIZE), dep, link(false)), "nz_fill_beyer_queue");
                    dep = h;
                }
                check(nz_queued_beyer_cycle(ctx, heightMap->ptr, poolMap.ptr, streamMap.ptr, particleTrack.ptr, particleQueue, events,
                                            &ep, &tm, EVENT_LIMIT, res, dep, link(false)), "nz_queued_beyer_cycle");
                dep = h;
                check(nz_process_beyer_erosive_events(ctx, heightMap->ptr, poolMap.ptr, streamMap.ptr, particleTrack.ptr, events, &ep,
                                                      &tm, res, dep, link(false)), "nz_process_beyer_erosive_events");
                // CombineDependencies(ClearQueueJob, ErodeHeightMaps, UpdateFlowFromTrackJob), all behind the event reduction
                // (:408-412): the clear, then the two siblings as one call (the pile solver's launch carries the flow update's
                // workgroups); fuseSiblings = false: the two entries one after the other on the context's stream
                dep = h;
                check(nz_clear_particle_queue(ctx, particleQueue, dep, link(false)), "nz_clear_particle_queue");
                dep = h;
                if (fuseSiblings) {
                    check(nz_erode_height_maps_and_flow(ctx, heightMap->ptr, events, poolMap.ptr, streamMap.ptr, particleTrack.ptr, &ep,
                                                        &tm, res, dep, link(false)), "nz_erode_height_maps_and_flow");
                } else {
                    check(nz_erode_height_maps(ctx, heightMap->ptr, events, &ep, &tm, res, dep, link(false)), "nz_erode_height_maps");
                    dep = h;
                    check(nz_update_flow_from_track(ctx, poolMap.ptr, streamMap.ptr, particleTrack.ptr, ep.FLOW_LOSS_RATE,
                                                    ep.SURFACE_EVAPORATION_RATE, (float)tm.HEIGHT, res, dep, link(false)), "nz_update_flow_from_track");
                }
                dep = h;
                check(nz_pool_automata_job(ctx, poolMap.ptr, heightMap->ptr, particleQueue, &ep, &tm, es.WATER_STEPS, res,
                                           performErosion ? 1 : 0, dep, link(last)), "nz_pool_automata_job");
            }
        }
        jobHandle = JobHandle{ctx, h};
        particleGenerationID += 1;  // Update() :341
        return jobHandle;
    }

    nz_ctx *ctx;
    bool fewHandles = true;         // false: a handle out of every job, as the reference schedules them (one event record each)
    bool fuseSiblings = true;       // ErodeHeightMaps + UpdateFlowFromTrackJob as one call (nz_erode_height_maps_and_flow)
    DeviceTile *heightMap;
    nz_tile_set_meta tileMeta;
    ErosionSettings erosionSettings;
    bool performErosion;
    int res, QUEUE_SIZE = 0, particleGenerationID = 0, EVENT_LIMIT = 1500;
    DeviceTile poolMap, streamMap, particleTrack;
    nz_particle_queue *particleQueue = nullptr;
    nz_erosive_events *events = nullptr;
    JobHandle jobHandle;
};


// The stock stage list NoiseStage -> [KernelFilterStage] -> [FlowMapStage] -> [ErosionStage] (README.md:23-32), all on one
// context, as nz_terrain_params (what ShardedPipeline hands to nz_sharded_create); false if the list is anything else.
inline bool stockListParams(const std::vector<PipelineStage *> &stages, nz_terrain_params *tp, NoiseStage **noise) {
    if (stages.empty()) return false;
    auto *n = dynamic_cast<NoiseStage *>(stages[0]);
    if (!n) return false;
    KernelFilterStage *f = nullptr;
    FlowMapStage *w = nullptr;
    ErosionStage *e = nullptr;
    int k = 0;  // the optional stages must come in this order, each at most once
    for (size_t i = 1; i < stages.size(); i++) {
        PipelineStage *s = stages[i];
        if (s->Context() != n->Context()) return false;
        if (k < 1 && typeid(*s) == typeid(KernelFilterStage)) { f = static_cast<KernelFilterStage *>(s); k = 1; }
        else if (k < 2 && typeid(*s) == typeid(FlowMapStage)) { w = static_cast<FlowMapStage *>(s); k = 2; }
        else if (k < 3 && typeid(*s) == typeid(ErosionStage)) { e = static_cast<ErosionStage *>(s); k = 3; }
        else return false;
    }
    if (typeid(*n) != typeid(NoiseStage) || (f && f->filter == NZ_SOBEL3_2D)) return false;
    *tp = nz_terrain_params{};
    tp->noiseType = (int)n->noiseType;
    tp->hurst = n->hurst; tp->startingAmplitude = n->startingAmplitude; tp->stepdown = n->stepdown; tp->detuneRate = n->detuneRate;
    tp->octaves = n->octaves; tp->noiseSize = n->noiseSize;
    tp->filter = f ? f->filter : 0; tp->filterIterations = f ? f->iterations : 0;
    tp->flowIterations = w ? w->iterations : 0; tp->normMin = w ? w->normMin : 0.f; tp->normMax = w ? w->normMax : 0.f;
    tp->erosionIterations = e ? e->iterations : 0;
    if (noise) *noise = n;
    return true;
}

inline bool BasePipeline::RegeneratesItsTile() const {
    // a NoiseStage or one derived from it (ShapedNoiseStage), as isinstance in the Python host and `is` in the C# one
    return !stage_instances.empty() && dynamic_cast<NoiseStage *>(stage_instances[0]) != nullptr;
}

// ---- one large grid over the GPUs of a node (new-framework feature; include/noize_hip.h, nz_comm.cpp) -------------------
// The reference's host asks for one tile at a time (BasePipeline.Schedule, Pipeline/Executable/Pipeline.cs:104-128;
// Scripts/MeshTileGenerator.cs:166-192); a grid larger than a tile is cut into row stripes, one process per GPU, and the
// stock stage list runs on all of them with RCCL neighbour halo exchange.
class Comm {  // nz_comm: ncclCommInitRank on the context's device + the exchanges' stream
  public:
    static std::array<uint8_t, NZ_COMM_ID_BYTES> UniqueId() {  // by ONE rank; the bytes travel out of band
        std::array<uint8_t, NZ_COMM_ID_BYTES> id{};
        check(nz_comm_unique_id(id.data()), "nz_comm_unique_id");
        return id;
    }
    Comm(nz_ctx *ctx, const std::array<uint8_t, NZ_COMM_ID_BYTES> &id, int rank, int world) {
        check(nz_comm_init(ctx, id.data(), rank, world, &h), "nz_comm_init");
    }
    // nz_comm_destroy refuses while ShardedPipelines still hold the communicator (destroy them first -- objects declared
    // after the Comm are, by the language's order).  Close() reports that; the destructor can only say so.
    void Close() {
        if (!h) return;
        check(nz_comm_destroy(h), "nz_comm_destroy");
        h = nullptr;
    }
    ~Comm() {
        if (h && nz_comm_destroy(h) != NZ_OK)
            std::fprintf(stderr, "noize::Comm: communicator leaked (%s)\n", nz_last_error());
    }
    Comm(const Comm &) = delete;
    Comm &operator=(const Comm &) = delete;
    int Rank() const { return nz_comm_rank(h); }
    int World() const { return nz_comm_world(h); }
    nz_comm *h = nullptr;
};

class ShardedPipeline {
  public:
    // `stages`: the stock list (stockListParams); comm may be null on one rank (device copies instead of RCCL);
    // stripes = 0: one per rank
    ShardedPipeline(nz_ctx *ctx, Comm *comm, const std::vector<PipelineStage *> &stages, int grows, int cols, int stripes = 0,
                    int haloMode = NZ_HALO_EXCHANGE, int overlap = 0, int xpos = 0, int zpos = 0)
        : ctx(ctx) {
        nz_terrain_params tp{};
        if (!stockListParams(stages, &tp, nullptr)) throw std::runtime_error("ShardedPipeline: not the stock stage list");
        nz_sharded_desc d{};
        d.grows = grows;
        d.cols = cols;
        d.stripes = stripes > 0 ? stripes : (comm ? comm->World() : 1);
        d.haloMode = haloMode;
        d.overlap = overlap;
        d.xpos = xpos;
        d.zpos = zpos;
        check(nz_sharded_create(ctx, comm ? comm->h : nullptr, &d, &tp, &h), "nz_sharded_create");
    }
    ~ShardedPipeline() { nz_sharded_destroy(h); }
    ShardedPipeline(const ShardedPipeline &) = delete;
    ShardedPipeline &operator=(const ShardedPipeline &) = delete;
    int LocalStripes() const { return nz_sharded_local_stripes(h); }
    JobHandle Schedule(JobHandle dependency = JobHandle()) {  // one pass over every local stripe (enqueue only)
        nz_handle out = 0;
        check(nz_sharded_pipeline(ctx, h, nullptr, dependency.id, &out), "nz_sharded_pipeline");
        return JobHandle{ctx, out};
    }
    // local stripe i: first owned global row, owned rows, host copy of them (rows x cols floats)
    int OwnedRows(int i, int *firstGlobalRow = nullptr) const {
        nz_stripe st{};
        check(nz_sharded_stripe(h, i, &st, nullptr, nullptr), "nz_sharded_stripe");
        if (firstGlobalRow) *firstGlobalRow = st.grow0 + st.own0;
        return st.own1 - st.own0;
    }
    void CopyOwnedRows(int i, float *host) const {
        nz_stripe st{};
        float *res = nullptr;
        check(nz_sharded_stripe(h, i, &st, nullptr, &res), "nz_sharded_stripe");
        const size_t n = (size_t)(st.own1 - st.own0) * st.cols;
        nz_handle done = 0;
        check(nz_tile_download(ctx, res + (size_t)st.own0 * st.cols, host, n, 0, &done), "nz_tile_download");
        check(nz_handle_wait(ctx, done), "nz_handle_wait");
    }
    nz_ctx *ctx;
    nz_sharded *h = nullptr;
};

}  // namespace noize
