// host_demo_stages.hpp -- host_demo's `stage` mode: every stage class of noize_pipeline.hpp run on the device, one scenario
// per class, on planes the caller supplies, so that the test suite can hold the C++ host against the models it holds the
// Python host against (tests/test_gpu_cpp_host_stages.py; the scenario names are pinned by tests/test_cpp_host_stages.py).
//
//   host_demo <res> <out.bin> stage <StageName> <in.f32>
//   host_demo 0 - stage --list
//
// <in.f32> is raw little-endian float32, the planes a scenario documents back to back; <res> is not used.  Every plane a
// scenario reads back goes to <out.bin> back to back, one stdout line per plane in file order,
//   plane <name> <f32|i32|u8> <elements>
// and every scalar -- an accessor's value, a fact about which plane is which -- goes to stdout as
//   value <name> <int>
// A name is "<step>.<what>"; the steps are the letters of the comments below.  --list, an unknown name and an input file
// of the wrong size are answered before a context is created.
#pragma once

#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <functional>
#include <memory>
#include <string>
#include <type_traits>
#include <vector>

#include "noize_pipeline.hpp"

namespace stage_demo {
using namespace noize;

constexpr size_t N97 = 97 * 97, N96 = 96 * 96, N32 = 32 * 32, N33 = 33 * 33;
constexpr float SEA = 0.4f, OFF = -3.402823466e+38f, SENTINEL = -123.5f;
constexpr int AMPLE = 600;  // a pass budget no tile of the scenarios comes near

// ---- the run: the input planes, the output file, the two kinds of stdout line ------------------------------------------
struct Run {
    nz_ctx *ctx = nullptr;
    std::vector<float> in;
    size_t at = 0;
    FILE *out = nullptr;

    const float *take(size_t n) {
        if (at + n > in.size()) throw std::runtime_error("the input file is too short");
        const float *p = in.data() + at;
        at += n;
        return p;
    }
    std::unique_ptr<DeviceTile> tile(const float *host, size_t n) {
        std::unique_ptr<DeviceTile> t(new DeviceTile(ctx, n));
        t->CopyFrom(host);
        return t;
    }
    std::unique_ptr<DeviceTile> filled(size_t n, float v) {
        const std::vector<float> host(n, v);
        return tile(host.data(), n);
    }
    void value(const std::string &name, long v) { std::printf("value %s %ld\n", name.c_str(), v); }
    void put(const std::string &name, const char *type, const void *host, size_t elements, size_t bytes) {
        if (std::fwrite(host, 1, bytes, out) != bytes) throw std::runtime_error("write failed");
        std::printf("plane %s %s %zu\n", name.c_str(), type, elements);
    }
    std::vector<float> download(const void *dev, size_t floats) {
        std::vector<float> host(floats);
        if (floats) {
            check(nz_tile_download(ctx, static_cast<const float *>(dev), host.data(), floats, 0, nullptr), "nz_tile_download");
            check(nz_ctx_synchronize(ctx), "nz_ctx_synchronize");
        }
        return host;
    }
    void f32(const std::string &name, const float *dev, size_t n) { put(name, "f32", download(dev, n).data(), n, 4 * n); }
    void i32(const std::string &name, const int32_t *dev, size_t n) { put(name, "i32", download(dev, n).data(), n, 4 * n); }
    void u8(const std::string &name, const uint8_t *dev, size_t n) { put(name, "u8", download(dev, (n + 3) / 4).data(), n, n); }
    // an accessor that may be empty: "<name>_null 0/1", and the plane when there is one
    void f32_or_null(const std::string &name, const float *dev, size_t n) {
        value(name + "_null", dev == nullptr);
        if (dev) f32(name, dev, n);
    }
    void i32_or_null(const std::string &name, const int32_t *dev, size_t n) {
        value(name + "_null", dev == nullptr);
        if (dev) i32(name, dev, n);
    }
    void u8_or_null(const std::string &name, const uint8_t *dev, size_t n) {
        value(name + "_null", dev == nullptr);
        if (dev) u8(name, dev, n);
    }
};

// a payload and the planes behind it: one tile, or `count` tiles back to back as a GeneratorDataBatch; `second` is the
// WRITE plane of a pair, filled with SENTINEL
struct Payload {
    std::unique_ptr<DeviceTile> first, second, positions;
    GeneratorData single;
    GeneratorDataBatch batch;
    bool many = false;
    GeneratorData *gd() { return many ? &batch : &single; }
    size_t cells() { return first->Length; }
};

inline std::unique_ptr<Payload> payload(Run &r, const float *host, int res, int count, bool pair = false,
                                        const std::vector<int32_t> &pos = {}) {
    std::unique_ptr<Payload> p(new Payload);
    const size_t n = (size_t)count * res * res;
    p->first = host ? r.tile(host, n) : r.filled(n, SENTINEL);
    if (pair) p->second = r.filled(n, SENTINEL);
    p->many = count > 1;
    GeneratorData *g = p->gd();
    g->uuid = "stage-demo";
    g->data = p->first.get();
    g->write = p->second.get();
    g->resolution = res;
    if (p->many) {
        p->batch.count = count;
        if (!pos.empty()) {
            p->positions = r.tile(reinterpret_cast<const float *>(pos.data()), pos.size());
            p->batch.positions = reinterpret_cast<const int32_t *>(p->positions->ptr);
            p->batch.hostPositions = pos;
        }
    }
    return p;
}

// one stage as a BasePipeline of its own: Enqueue, RunToCompletion, a counted completion callback.  The pipeline lives as
// long as the stage does (Setup() hooks it into the stage).  -> the payload the pipeline ended with
struct Driver {
    BasePipeline pipe;
    int completed = 0;
    StageIO *last = nullptr;
    explicit Driver(std::vector<PipelineStage *> stages) : pipe(std::move(stages)) {}
    StageIO *run(StageIO *d) {
        const int before = completed;
        pipe.Enqueue(d, nullptr, [this](StageIO *o) {
            completed++;
            last = o;
        });
        pipe.RunToCompletion();
        if (completed != before + 1) throw std::runtime_error("completeAction did not fire exactly once");
        return last;
    }
};

// the pair facts of step d: which plane `data` is, and that the pair is still the two planes it was
inline void pair_facts(Run &r, const std::string &step, Payload &p) {
    GeneratorData *g = p.gd();
    r.value(step + ".data_is_first", g->data == p.first.get());
    if (p.second)
        r.value(step + ".pair_kept", (g->data == p.first.get() && g->write == p.second.get()) ||
                                         (g->data == p.second.get() && g->write == p.first.get()));
    else
        r.value(step + ".write_null", g->write == nullptr);
}

// ---- the terrain scenarios' input: h97, h96, 9 x h32, 3 x h33, ties97, then four 97^2 option planes m0..m3 whose meaning
//      the scenario states -------------------------------------------------------------------------------------------------
constexpr size_t TERRAIN_FLOATS = 6 * N97 + N96 + 9 * N32 + 3 * N33;
struct Terrain {
    const float *h97, *h96, *h32, *h33, *ties, *m[4];
    explicit Terrain(Run &r) {
        h97 = r.take(N97);
        h96 = r.take(N96);
        h32 = r.take(9 * N32);
        h33 = r.take(3 * N33);
        ties = r.take(N97);
        for (auto &p : m) p = r.take(N97);
    }
};

// the accessors of a stage, each under "<step>."
inline void dump(Run &r, const std::string &s, HydraulicErosionStage &st) {
    r.f32_or_null(s + ".water", st.water(), st.waterLength());
    r.f32_or_null(s + ".wear", st.wear(), st.waterLength());
    r.f32_or_null(s + ".deposits", st.deposits(), st.waterLength());
}
inline void dump(Run &r, const std::string &s, FluvialErosionStage &st) {
    r.f32_or_null(s + ".drainage", st.drainage(), st.drainageLength());
}
template <class S>
void dump_drainage(Run &r, const std::string &s, S &st) {
    r.f32_or_null(s + ".drainage", st.drainage(), st.drainageLength());
    r.value(s + ".passes", st.passes());
    r.value(s + ".converged", st.converged());
    r.value(s + ".work_floats", (long)st.workLength());
}
inline void dump(Run &r, const std::string &s, DrainageAreaStage &st) { dump_drainage(r, s, st); }
inline void dump(Run &r, const std::string &s, MfdDrainageStage &st) { dump_drainage(r, s, st); }
inline void dump(Run &r, const std::string &s, WatershedStage &st) {
    r.i32_or_null(s + ".basin", st.basin(), st.cells());
    r.f32_or_null(s + ".length", st.flowLength(), st.cells());
    r.u8_or_null(s + ".receivers", st.receivers(), st.cells());
    r.value(s + ".passes", st.passes());
    r.value(s + ".converged", st.converged());
    r.value(s + ".work_floats", (long)st.workLength());
}
inline void dump(Run &r, const std::string &s, StreamOrderStage &st) {
    r.u8_or_null(s + ".order", st.order(), st.cells());
    r.i32_or_null(s + ".links", st.links(), st.cells());
    r.value(s + ".passes", st.passes());
    r.value(s + ".converged", st.converged());
    r.value(s + ".work_floats", (long)st.workLength());
}
template <class S>
void dump_implicit(Run &r, const std::string &s, S &st) {
    r.f32_or_null(s + ".drainage", st.drainage(), st.cells());
    r.value(s + ".steps", st.steps());
    r.value(s + ".passes", st.passes());
    r.value(s + ".converged", st.converged());
    r.value(s + ".work_floats", (long)st.workLength());
}
inline void dump(Run &r, const std::string &s, ImplicitFluvialStage &st) { dump_implicit(r, s, st); }
inline void dump(Run &r, const std::string &s, MfdFluvialStage &st) { dump_implicit(r, s, st); }
inline void dump(Run &r, const std::string &s, HillslopeDiffusionStage &st) { r.value(s + ".work_floats", (long)st.workLength()); }

// one payload through the stage's pipeline: "<step>.height" is the payload's `data` afterwards, then the accessors
template <class S>
std::unique_ptr<Payload> through(Run &r, Driver &d, S &st, const std::string &step, const float *host, int res, int count,
                                 bool pair = false) {
    auto p = payload(r, host, res, count, pair);
    if (d.run(p->gd()) != p->gd()) throw std::runtime_error("the stage handed on another payload");
    r.f32(step + ".height", p->gd()->data->ptr, p->cells());
    dump(r, step, st);
    return p;
}

// step e: the same instance on 96^2, on 9 x 32^2 (equal length, other tiling), then on 3 x 33^2; `need` is the entry's own
// size query, printed next to the stage's work_floats
template <class S>
void tilings(Run &r, Driver &d, S &st, const Terrain &in, const std::function<size_t(int, int)> &need) {
    through(r, d, st, "e96", in.h96, 96, 1);
    r.value("e96.work_need", (long)need(96, 1));
    through(r, d, st, "e32", in.h32, 32, 9);
    r.value("e32.work_need", (long)need(32, 9));
    through(r, d, st, "e33", in.h33, 33, 3);
    r.value("e33.work_need", (long)need(33, 3));
}

// step g: OnDestroy empties the accessors, and one more payload works
template <class S>
void destroyed(Run &r, Driver &d, S &st, const Terrain &in) {
    st.OnDestroy();
    dump(r, "g", st);
    through(r, d, st, "h", in.h33, 33, 1);
}

// step d: a WRITE plane with an even and an odd count, then no WRITE plane with an odd count
template <class S>
void plane_pair(Run &r, Driver &d, S &st, const Terrain &in) {
    for (int n : {2, 3}) {
        st.iterations = n;
        const std::string step = "d" + std::to_string(n);
        auto p = through(r, d, st, step, in.h97, 97, 1, true);
        pair_facts(r, step, *p);
    }
    st.iterations = 3;
    auto p = through(r, d, st, "d1", in.h97, 97, 1, false);
    pair_facts(r, "d1", *p);
}

// HydraulicErosionStage.  m0: rainMap, m1: hardness.  a: accessors; b: defaults but 8 iterations; t: the tie tile;
// c: Open border, both maps, the masks, capacity 2, 7 iterations; c2: the masks off again; d: the pair (plain entries);
// e: tilings at 4 iterations; g: OnDestroy, h: one more payload
inline void hydraulic(Run &r) {
    const Terrain in(r);
    HydraulicErosionStage st(r.ctx);
    Driver d({&st});
    dump(r, "a", st);
    st.iterations = 8;
    through(r, d, st, "b", in.h97, 97, 1);
    through(r, d, st, "t", in.ties, 97, 1);
    auto rain = r.tile(in.m[0], N97), hard = r.tile(in.m[1], N97);
    st.iterations = 7;
    st.capacity = 2.f;
    st.border = HydraulicBorder::Open;
    st.rainMap = rain.get();
    st.hardness = hard.get();
    st.recordMasks = true;
    through(r, d, st, "c", in.h97, 97, 1);
    st.recordMasks = false;
    through(r, d, st, "c2", in.h97, 97, 1);
    r.f32("c2.rainMap", rain->ptr, N97);
    r.f32("c2.hardness", hard->ptr, N97);
    st.capacity = 1.f;
    st.border = HydraulicBorder::Closed;
    st.rainMap = st.hardness = nullptr;
    plane_pair(r, d, st, in);
    st.iterations = 4;
    through(r, d, st, "e96", in.h96, 96, 1);
    through(r, d, st, "e32", in.h32, 32, 9);
    through(r, d, st, "e33", in.h33, 33, 3);
    destroyed(r, d, st, in);
}

// FluvialErosionStage.  m0: rainMap, m1: hardness, m2: upliftMap, m3: drainageIn.  b: defaults but 8 iterations;
// c: every map, a sea, erodibility .1, uplift .004, dt .5, rain .75, 5 iterations; d; e at 4 iterations; g, h
inline void fluvial(Run &r) {
    const Terrain in(r);
    FluvialErosionStage st(r.ctx);
    Driver d({&st});
    dump(r, "a", st);
    st.iterations = 8;
    through(r, d, st, "b", in.h97, 97, 1);
    through(r, d, st, "t", in.ties, 97, 1);
    std::unique_ptr<DeviceTile> m[4];
    for (int k = 0; k < 4; k++) m[k] = r.tile(in.m[k], N97);
    st.iterations = 5;
    st.erodibility = .1f;
    st.uplift = .004f;
    st.dt = .5f;
    st.rain = .75f;
    st.seaLevel = SEA;
    st.rainMap = m[0].get();
    st.hardness = m[1].get();
    st.upliftMap = m[2].get();
    st.drainageIn = m[3].get();
    through(r, d, st, "c", in.h97, 97, 1);
    for (int k = 0; k < 4; k++) r.f32("c.m" + std::to_string(k), m[k]->ptr, N97);
    st.erodibility = .05f;
    st.uplift = .002f;
    st.dt = st.rain = 1.f;
    st.seaLevel = OFF;
    st.rainMap = st.hardness = st.upliftMap = st.drainageIn = nullptr;
    plane_pair(r, d, st, in);
    st.iterations = 4;
    through(r, d, st, "e96", in.h96, 96, 1);
    through(r, d, st, "e32", in.h32, 32, 9);
    through(r, d, st, "e33", in.h33, 33, 3);
    destroyed(r, d, st, in);
}

// DrainageAreaStage and MfdDrainageStage.  m0: rainMap.  b: defaults; t: the tie tile; c: rain .5, a sea, the rain map, a
// caller's `out` plane, an ample budget (and exponent 4); c2: `out` and the map off again; e: tilings (exponent 2);
// f: a budget of 2; g, h
template <class S>
void drainage_like(Run &r, const std::function<size_t(int, int)> &need) {
    const Terrain in(r);
    S st(r.ctx);
    Driver d({&st});
    dump(r, "a", st);
    through(r, d, st, "b", in.h97, 97, 1);
    through(r, d, st, "t", in.ties, 97, 1);
    auto rain = r.tile(in.m[0], N97), out = r.filled(N97, SENTINEL);
    st.rain = .5f;
    st.seaLevel = SEA;
    st.maxPasses = AMPLE;
    st.rainMap = rain.get();
    st.out = out.get();
    if constexpr (std::is_same<S, MfdDrainageStage>::value) st.exponent = 4;
    through(r, d, st, "c", in.h97, 97, 1);
    r.value("c.drainage_is_out", st.drainage() == out->ptr);
    r.f32("c.rainMap", rain->ptr, N97);
    st.rainMap = nullptr;
    st.out = nullptr;
    through(r, d, st, "c2", in.h97, 97, 1);
    r.value("c2.drainage_is_out", st.drainage() == out->ptr);
    r.f32("c2.out", out->ptr, N97);  // the caller's plane keeps what step c left in it
    st.rain = 1.f;
    st.seaLevel = OFF;
    st.maxPasses = 0;
    if constexpr (std::is_same<S, MfdDrainageStage>::value) st.exponent = 2;
    tilings(r, d, st, in, need);
    st.maxPasses = 2;
    through(r, d, st, "f", in.h97, 97, 1);
    st.maxPasses = 0;
    destroyed(r, d, st, in);
}

// WatershedStage.  b: defaults (labels and length); t; c: receivers, no length, cellSize .3, a sea, an ample budget;
// c2: length on and receivers off again; e: tilings with both planes; f: a budget of 2; g, h
inline void watershed(Run &r) {
    const Terrain in(r);
    WatershedStage st(r.ctx);
    Driver d({&st});
    dump(r, "a", st);
    through(r, d, st, "b", in.h97, 97, 1);
    through(r, d, st, "t", in.ties, 97, 1);
    st.recordReceivers = true;
    st.length = false;
    st.cellSize = .3f;
    st.seaLevel = SEA;
    st.maxPasses = AMPLE;
    through(r, d, st, "c", in.h97, 97, 1);
    st.recordReceivers = false;
    st.length = true;
    through(r, d, st, "c2", in.h97, 97, 1);
    st.cellSize = 1.f;
    st.seaLevel = OFF;
    st.maxPasses = 0;
    st.recordReceivers = true;
    tilings(r, d, st, in, [&](int res, int count) { return nz_watershed_work_floats(res, count, 1); });
    st.recordReceivers = false;
    st.maxPasses = 2;
    through(r, d, st, "f", in.h97, 97, 1);
    st.maxPasses = 0;
    destroyed(r, d, st, in);
}

// StreamOrderStage.  m0: a drainage plane of h97.  b: defaults (order only, every cell a channel); t; c: the drainage
// plane with threshold 6, a sea, links, an ample budget; c2: links off again; e: tilings with links, no drainage plane;
// f: a budget of 2 with links; g, h
inline void stream_order(Run &r) {
    const Terrain in(r);
    StreamOrderStage st(r.ctx);
    Driver d({&st});
    dump(r, "a", st);
    through(r, d, st, "b", in.h97, 97, 1);
    through(r, d, st, "t", in.ties, 97, 1);
    auto area = r.tile(in.m[0], N97);
    st.drainage = area.get();
    st.threshold = 6.f;
    st.seaLevel = SEA;
    st.recordLinks = true;
    st.maxPasses = AMPLE;
    through(r, d, st, "c", in.h97, 97, 1);
    r.f32("c.drainage", area->ptr, N97);
    st.recordLinks = false;
    through(r, d, st, "c2", in.h97, 97, 1);
    st.drainage = nullptr;
    st.threshold = 0.f;
    st.seaLevel = OFF;
    st.maxPasses = 0;
    st.recordLinks = true;
    tilings(r, d, st, in, [&](int res, int count) { return nz_stream_order_work_floats(res, count, 1); });
    st.maxPasses = 2;
    through(r, d, st, "f", in.h97, 97, 1);
    st.maxPasses = 0;
    destroyed(r, d, st, in);
}

// ImplicitFluvialStage and MfdFluvialStage.  m0: rainMap, m1: hardness, m2: upliftMap, m3: the heights of step f2, one
// long winding channel.  b: defaults; t; c: the three
// maps, a sea, erodibility .1, uplift .01, dt 20, rain 2, an ample budget (MfdFluvialStage: exponent 4); cm
// (ImplicitFluvialStage alone): the same with routing = Multiple, flowExponent = 4; d: the pair at dt 50; e: tilings at
// 2 iterations, dt 50; f: a budget of 2 at 2 iterations (fm: with routing = Multiple); f2: see there -- the drainage series
// runs out, the solve must not proceed; g, h
template <class S>
void implicit_like(Run &r, const std::function<size_t(int, int)> &need) {
    constexpr bool mfd = std::is_same<S, MfdFluvialStage>::value;
    const Terrain in(r);
    S st(r.ctx);
    Driver d({&st});
    dump(r, "a", st);
    through(r, d, st, "b", in.h97, 97, 1);
    through(r, d, st, "t", in.ties, 97, 1);
    std::unique_ptr<DeviceTile> m[3];
    for (int k = 0; k < 3; k++) m[k] = r.tile(in.m[k], N97);
    st.erodibility = .1f;
    st.uplift = .01f;
    st.dt = 20.f;
    st.rain = 2.f;
    st.seaLevel = SEA;
    st.maxPasses = AMPLE;
    st.rainMap = m[0].get();
    st.hardness = m[1].get();
    st.upliftMap = m[2].get();
    if constexpr (mfd) st.exponent = 4;
    through(r, d, st, "c", in.h97, 97, 1);
    if constexpr (!mfd) {
        st.routing = FlowRouting::Multiple;
        st.flowExponent = 4;
        through(r, d, st, "cm", in.h97, 97, 1);
        st.routing = FlowRouting::Steepest;
    }
    for (int k = 0; k < 3; k++) r.f32("c.m" + std::to_string(k), m[k]->ptr, N97);
    st.erodibility = .05f;
    st.uplift = .002f;
    st.dt = 50.f;
    st.rain = 1.f;
    st.seaLevel = OFF;
    st.maxPasses = 0;
    st.rainMap = st.hardness = st.upliftMap = nullptr;
    if constexpr (mfd) st.exponent = 2;
    plane_pair(r, d, st, in);
    st.iterations = 2;
    tilings(r, d, st, in, need);
    st.maxPasses = 2;
    through(r, d, st, "f", in.h97, 97, 1);
    if constexpr (!mfd) {  // fm: the same with the multiple-flow drainage in front
        st.routing = FlowRouting::Multiple;
        through(r, d, st, "fm", in.h97, 97, 1);
        st.routing = FlowRouting::Steepest;
    }
    // f2: the long chain m3 at a budget of 3 with erodibility 0 -- a solve that is done at once, if it is told to proceed
    st.maxPasses = 3;
    st.iterations = 1;
    st.erodibility = 0.f;
    st.uplift = .01f;
    st.dt = 3.f;
    through(r, d, st, "f2", in.m[3], 97, 1);
    st.erodibility = .05f;
    st.uplift = .002f;
    st.dt = 50.f;
    st.maxPasses = 0;
    destroyed(r, d, st, in);
}

// HillslopeDiffusionStage.  b: defaults; t; c: diffusivity 2.5, dt 4, 3 iterations; e: tilings; g, h
inline void hillslope(Run &r) {
    const Terrain in(r);
    HillslopeDiffusionStage st(r.ctx);
    Driver d({&st});
    dump(r, "a", st);
    through(r, d, st, "b", in.h97, 97, 1);
    through(r, d, st, "t", in.ties, 97, 1);
    st.diffusivity = 2.5f;
    st.dt = 4.f;
    st.iterations = 3;
    through(r, d, st, "c", in.h97, 97, 1);
    tilings(r, d, st, in, [](int res, int count) { return nz_hillslope_diffusion_work_floats(res, count); });
    destroyed(r, d, st, in);
}

// ---- the one-call stages: s1, s2, ... are payloads through ONE instance (and one pipeline of that one stage), the members
//      changed in between as the comments say; a plane "<step>.data" is the payload's `data` afterwards -------------------

// the payload a pipeline ended with, as GeneratorData: its plane and what TransformData made of the fields
inline void result(Run &r, const std::string &step, StageIO *o) {
    auto *g = dynamic_cast<GeneratorData *>(o);
    if (!g) throw std::runtime_error("the pipeline did not end with a GeneratorData");
    const int count = tile_count(g);
    r.f32(step + ".data", g->data->ptr, (size_t)count * g->resolution * g->resolution);
    r.value(step + ".resolution", g->resolution);
    r.value(step + ".count", count);
    r.value(step + ".length", (long)g->data->Length);
    if (auto *b = dynamic_cast<GeneratorDataBatch *>(g)) {
        if (b->positions) r.i32(step + ".positions", b->positions, 2 * (size_t)count);
    } else {
        r.value(step + ".xpos", g->xpos);
        r.value(step + ".zpos", g->zpos);
    }
}

// ConstantStage.  Input: a (130^2), b (33^2).  s1: MULTIPLY by .37 on a; s2: BINARIZE at .37 on a; s3: MULTIPLY by -1.5 on b
inline void constant(Run &r) {
    const float *a = r.take(130 * 130), *b = r.take(N33);
    ConstantStage st(r.ctx);
    Driver d({&st});
    st.value = .37f;
    auto p1 = payload(r, a, 130, 1);
    result(r, "s1", d.run(p1->gd()));
    st.operation = 1;
    auto p2 = payload(r, a, 130, 1);
    result(r, "s2", d.run(p2->gd()));
    st.operation = 0;
    st.value = -1.5f;
    auto p3 = payload(r, b, 33, 1);
    result(r, "s3", d.run(p3->gd()));
    st.OnDestroy();
}

// CurveStage.  Input: a (130^2), b (33^2).  s1: smoothstep t * t * (3 - 2 t) in 64 samples on a; s2: the same instance, same
// length; s3: 1.5 t - 0.1 in 7 samples on b -- the table is extracted again when the length changes
inline void curve(Run &r) {
    const float *a = r.take(130 * 130), *b = r.take(N33);
    CurveStage st(r.ctx);
    Driver d({&st});
    st.samples = 64;
    st.unityCurve = [](float t) { return t * t * (3.0f - 2.0f * t); };
    auto p1 = payload(r, a, 130, 1);
    result(r, "s1", d.run(p1->gd()));
    auto p2 = payload(r, a, 130, 1);
    result(r, "s2", d.run(p2->gd()));
    st.samples = 7;
    st.unityCurve = [](float t) { return 1.5f * t - 0.1f; };
    auto p3 = payload(r, b, 33, 1);
    result(r, "s3", d.run(p3->gd()));
    st.OnDestroy();
}

// StageThermalErosion.  Input: a (65^2), b (33^2).  s1: 3 iterations, talus 20, increment .25, ratio .3 on a; s2: 2 iterations,
// talus 80, increment .5, ratio 2 on b
inline void thermal(Run &r) {
    const float *a = r.take(65 * 65), *b = r.take(N33);
    StageThermalErosion st(r.ctx);
    Driver d({&st});
    st.iterations = 3;
    st.talus = 20;
    st.increment = .25f;
    st.meshHeightWidthRatio = .3f;
    auto p1 = payload(r, a, 65, 1);
    result(r, "s1", d.run(p1->gd()));
    st.iterations = 2;
    st.talus = 80;
    st.increment = .5f;
    st.meshHeightWidthRatio = 2.f;
    auto p2 = payload(r, b, 33, 1);
    result(r, "s2", d.run(p2->gd()));
}

// CropStage.  Input: a (150^2).  s1: cropped to 64^2; s2: to 161^2, larger than the input; "<step>.input" is the input after
inline void crop(Run &r) {
    const float *a = r.take(150 * 150);
    CropStage st(r.ctx);
    Driver d({&st});
    auto src = r.tile(a, 150 * 150);
    for (int k = 0; k < 2; k++) {
        const int res = k == 0 ? 64 : 161;
        const std::string step = "s" + std::to_string(k + 1);
        auto dst = r.filled((size_t)res * res, SENTINEL);
        DownsampleData dd;
        dd.uuid = "stage-demo";
        dd.data = dst.get();
        dd.inputData = src.get();
        dd.resolution = res;
        dd.inputResolution = 150;
        if (d.run(&dd) != &dd) throw std::runtime_error("the stage handed on another payload");
        r.f32(step + ".data", dst->ptr, (size_t)res * res);
        r.f32(step + ".input", src->ptr, 150 * 150);
    }
}

// StageGaussianBlur.  Input: a (90^2), b (3 x 37^2).  s1: 3 iterations, sigma 1, width 4 (an even width: limitWidth makes it 5)
// on a; s2: 2 iterations, sigma 5, width 13 on the batch b; s3: 2 iterations, sigma 3, width 9 on a with a WRITE plane
inline void gauss_blur(Run &r) {
    const float *a = r.take(90 * 90), *b = r.take(3 * 37 * 37);
    StageGaussianBlur st(r.ctx);
    Driver d({&st});
    st.iterations = 3;
    st.sigma = 1;
    st.width = 4;
    auto p1 = payload(r, a, 90, 1);
    result(r, "s1", d.run(p1->gd()));
    st.iterations = 2;
    st.sigma = 5;
    st.width = 13;
    auto p2 = payload(r, b, 37, 3);
    result(r, "s2", d.run(p2->gd()));
    st.sigma = 3;
    st.width = 9;
    auto p3 = payload(r, a, 90, 1, true);
    result(r, "s3", d.run(p3->gd()));
    pair_facts(r, "s3", *p3);
    st.OnDestroy();
}

// StageSmoothBlur (no batch form).  Input: a (77^2), b (33^2).  s1: 2 iterations, width 7 on a; s2: 1 iteration, width 25 on b;
// s3: 3 iterations, width 6 (even: 7) on a with a WRITE plane
inline void smooth_blur(Run &r) {
    const float *a = r.take(77 * 77), *b = r.take(N33);
    StageSmoothBlur st(r.ctx);
    Driver d({&st});
    st.iterations = 2;
    st.width = 7;
    auto p1 = payload(r, a, 77, 1);
    result(r, "s1", d.run(p1->gd()));
    st.iterations = 1;
    st.width = 25;
    auto p2 = payload(r, b, 33, 1);
    result(r, "s2", d.run(p2->gd()));
    st.iterations = 3;
    st.width = 6;
    auto p3 = payload(r, a, 77, 1, true);
    result(r, "s3", d.run(p3->gd()));
    pair_facts(r, "s3", *p3);
    st.OnDestroy();
}

// the positions of the noise scenarios' batch: three tiles of 64^2
inline std::vector<int32_t> noise_positions() { return {0, 0, -4096, 512, 300000, -70000}; }

// ShapedNoiseStage (no input plane).  s1: Simplex, ridged with offset .9 and gain 3.5, 6 octaves, 61^2 at (-2100, -777);
// s2: Cellular, billow, 9 octaves, a batch of three 64^2; s3: the same members on one 40^2 tile at (300000, 2000)
inline void shaped_noise(Run &r) {
    ShapedNoiseStage st(r.ctx);
    Driver d({&st});
    st.noiseType = FractalNoise::Simplex;
    st.hurst = .5938f;
    st.startingAmplitude = 1.3f;
    st.stepdown = 1.9168f;
    st.detuneRate = .0317f;
    st.octaves = 6;
    st.noiseSize = 97;
    st.shape = FractalShape::Ridged;
    st.ridgeOffset = .9f;
    st.ridgeGain = 3.5f;
    auto p1 = payload(r, nullptr, 61, 1);
    p1->single.xpos = -2100;
    p1->single.zpos = -777;
    result(r, "s1", d.run(p1->gd()));
    st.noiseType = FractalNoise::Cellular;
    st.hurst = .45f;
    st.startingAmplitude = 1.f;
    st.stepdown = 2.f;
    st.detuneRate = .01f;
    st.octaves = 9;
    st.noiseSize = 700;
    st.shape = FractalShape::Billow;
    st.ridgeOffset = 1.f;
    st.ridgeGain = 2.f;
    auto p2 = payload(r, nullptr, 64, 3, false, noise_positions());
    result(r, "s2", d.run(p2->gd()));
    auto p3 = payload(r, nullptr, 40, 1);
    p3->single.xpos = 300000;
    p3->single.zpos = 2000;
    result(r, "s3", d.run(p3->gd()));
}

// WarpedNoiseStage (no input plane).  s1: RotatedSimplex, ridged, 6 octaves, warp (-200, .25, 2), 40^2 at (-2100, -777);
// s2: Simplex, fBm, 9 octaves, warp (37.5, 1, 3), a batch of three 64^2; s3: the same members on one 61^2 tile at (0, 0)
inline void warped_noise(Run &r) {
    WarpedNoiseStage st(r.ctx);
    Driver d({&st});
    st.noiseType = FractalNoise::RotatedSimplex;
    st.hurst = .5938f;
    st.startingAmplitude = 1.3f;
    st.stepdown = 1.9168f;
    st.detuneRate = .0317f;
    st.octaves = 6;
    st.noiseSize = 97;
    st.shape = FractalShape::Ridged;
    st.warpStrength = -200.f;
    st.warpScale = .25f;
    st.warpOctaves = 2;
    auto p1 = payload(r, nullptr, 40, 1);
    p1->single.xpos = -2100;
    p1->single.zpos = -777;
    result(r, "s1", d.run(p1->gd()));
    st.noiseType = FractalNoise::Simplex;
    st.hurst = .45f;
    st.startingAmplitude = 1.f;
    st.stepdown = 2.f;
    st.detuneRate = .01f;
    st.octaves = 9;
    st.noiseSize = 700;
    st.shape = FractalShape::Fbm;
    st.warpStrength = 37.5f;
    st.warpScale = 1.f;
    st.warpOctaves = 3;
    auto p2 = payload(r, nullptr, 64, 3, false, noise_positions());
    result(r, "s2", d.run(p2->gd()));
    auto p3 = payload(r, nullptr, 61, 1);
    result(r, "s3", d.run(p3->gd()));
}

// the positions of the resample scenarios' batch: three tiles
inline std::vector<int32_t> resample_positions() { return {0, 0, 64, -64, -130, 7}; }

// UpsampleStage.  Input: a (37^2), b (3 x 16^2), base (74^2).  s1: factor 2, bilinear, `base` added, a at (6, -5); s2: factor 4,
// nearest, no base, the batch b (the output's positions are the input's times 4); s3: a NEW pair of stages, UpsampleStage(2,
// Catmull-Rom) then DownsampleStage(2) in one pipeline on a; "<step>.input" is the input plane afterwards
inline void upsample(Run &r) {
    const float *a = r.take(37 * 37), *b = r.take(3 * 16 * 16), *base = r.take(74 * 74);
    UpsampleStage st(r.ctx);
    Driver d({&st});
    auto plus = r.tile(base, 74 * 74);
    st.filter = ResampleFilter::Bilinear;
    st.base = plus.get();
    auto p1 = payload(r, a, 37, 1);
    p1->single.xpos = 6;
    p1->single.zpos = -5;
    result(r, "s1", d.run(p1->gd()));
    r.value("s1.data_is_output", static_cast<GeneratorData *>(d.last)->data == st.output());
    r.f32("s1.input", p1->first->ptr, 37 * 37);
    r.f32("s1.base", plus->ptr, 74 * 74);
    st.factor = 4;
    st.filter = ResampleFilter::Nearest;
    st.base = nullptr;
    auto p2 = payload(r, b, 16, 3, false, resample_positions());
    result(r, "s2", d.run(p2->gd()));
    r.f32("s2.input", p2->first->ptr, 3 * 16 * 16);
    UpsampleStage up(r.ctx);
    DownsampleStage down(r.ctx);
    Driver chain({&up, &down});
    auto p3 = payload(r, a, 37, 1);
    p3->single.xpos = 6;
    p3->single.zpos = -5;
    result(r, "s3", chain.run(p3->gd()));
    r.f32("s3.middle", up.output()->ptr, up.output()->Length);
    st.OnDestroy();
    r.value("g.output_null", st.output() == nullptr);
    chain.pipe.Destroy();
}

// DownsampleStage.  Input: a (64^2), b (3 x 32^2).  s1: factor 2, a at (6, -5); s2: factor 4, the batch b (positions floor-divided
// by 4); s3: a NEW pair of stages, DownsampleStage(2) then UpsampleStage(2) in one pipeline on a
inline void downsample(Run &r) {
    const float *a = r.take(64 * 64), *b = r.take(3 * 32 * 32);
    DownsampleStage st(r.ctx);
    Driver d({&st});
    auto p1 = payload(r, a, 64, 1);
    p1->single.xpos = 6;
    p1->single.zpos = -5;
    result(r, "s1", d.run(p1->gd()));
    r.value("s1.data_is_output", static_cast<GeneratorData *>(d.last)->data == st.output());
    r.f32("s1.input", p1->first->ptr, 64 * 64);
    st.factor = 4;
    auto p2 = payload(r, b, 32, 3, false, resample_positions());
    result(r, "s2", d.run(p2->gd()));
    r.f32("s2.input", p2->first->ptr, 3 * 32 * 32);
    DownsampleStage down(r.ctx);
    UpsampleStage up(r.ctx);
    Driver chain({&down, &up});
    auto p3 = payload(r, a, 64, 1);
    p3->single.xpos = 6;
    p3->single.zpos = -5;
    result(r, "s3", chain.run(p3->gd()));
    r.f32("s3.middle", down.output()->ptr, down.output()->Length);
    st.OnDestroy();
    r.value("g.output_null", st.output() == nullptr);
    chain.pipe.Destroy();
}

// MeshTileStage.  Input: a (35^2), b (4 x 72^2).  s1: the square grid, resolution 33 of 35 with margin 1, tile size 100 and
// height 25; s2: the overshoot mesh, a batch of four, resolution 64 of 72 with margin 4 -- the buffers follow the vertex count;
// "<step>.vertices": 12 floats per vertex, "<step>.indices"
inline void mesh(Run &r) {
    const float *a = r.take(35 * 35), *b = r.take(4 * 72 * 72);
    MeshTileStage st(r.ctx);
    Driver d({&st});
    MeshBuffers buffers;
    auto one = r.tile(a, 35 * 35), four = r.tile(b, 4 * 72 * 72);
    for (int k = 0; k < 2; k++) {
        const std::string step = "s" + std::to_string(k + 1);
        MeshStageData md;
        md.uuid = "stage-demo";
        md.mesh = &buffers;
        md.tileSize = 100.f;
        md.tileHeight = 25.f;
        md.data = k == 0 ? one.get() : four.get();
        md.resolution = k == 0 ? 33 : 64;
        md.inputResolution = k == 0 ? 35 : 72;
        md.marginPix = k == 0 ? 1 : 4;
        md.count = k == 0 ? 1 : 4;
        st.meshType = k == 0 ? NZ_MESH_SQUARE_GRID : NZ_MESH_OVERSHOOT_SQUARE_GRID;
        if (d.run(&md) != &md) throw std::runtime_error("the stage handed on another payload");
        r.value(step + ".vertex_count", (long)buffers.vertexCount);
        r.value(step + ".index_count", (long)buffers.indexCount);
        r.f32(step + ".vertices", buffers.vertices->ptr, buffers.vertexCount * 12);
        r.i32(step + ".indices", reinterpret_cast<const int32_t *>(buffers.indices->ptr), buffers.indexCount);
        r.f32(step + ".input", md.data->ptr, md.data->Length);
    }
}

// ---- the table, and the mode ----------------------------------------------------------------------------------------
struct Scenario {
    const char *name;
    size_t floats;  // of <in.f32>
    std::function<void(Run &)> run;
};

inline const std::vector<Scenario> &scenarios() {
    static const std::vector<Scenario> all = {
        {"HydraulicErosionStage", TERRAIN_FLOATS, hydraulic},
        {"FluvialErosionStage", TERRAIN_FLOATS, fluvial},
        {"DrainageAreaStage", TERRAIN_FLOATS,
         [](Run &r) { drainage_like<DrainageAreaStage>(r, [](int res, int n) { return nz_drainage_area_work_floats(res, n); }); }},
        {"MfdDrainageStage", TERRAIN_FLOATS,
         [](Run &r) { drainage_like<MfdDrainageStage>(r, [](int res, int n) { return nz_drainage_mfd_work_floats(res, n); }); }},
        {"WatershedStage", TERRAIN_FLOATS, watershed},
        {"StreamOrderStage", TERRAIN_FLOATS, stream_order},
        {"ImplicitFluvialStage", TERRAIN_FLOATS,
         [](Run &r) { implicit_like<ImplicitFluvialStage>(r, [](int res, int n) { return nz_fluvial_implicit_work_floats(res, n); }); }},
        {"MfdFluvialStage", TERRAIN_FLOATS,
         [](Run &r) { implicit_like<MfdFluvialStage>(r, [](int res, int n) { return nz_fluvial_implicit_mfd_work_floats(res, n); }); }},
        {"HillslopeDiffusionStage", TERRAIN_FLOATS, hillslope},
        {"ShapedNoiseStage", 0, shaped_noise},
        {"WarpedNoiseStage", 0, warped_noise},
        {"StageGaussianBlur", 90 * 90 + 3 * 37 * 37, gauss_blur},
        {"StageSmoothBlur", 77 * 77 + N33, smooth_blur},
        {"ConstantStage", 130 * 130 + N33, constant},
        {"CurveStage", 130 * 130 + N33, curve},
        {"StageThermalErosion", 65 * 65 + N33, thermal},
        {"CropStage", 150 * 150, crop},
        {"UpsampleStage", 37 * 37 + 3 * 16 * 16 + 74 * 74, upsample},
        {"DownsampleStage", 64 * 64 + 3 * 32 * 32, downsample},
        {"MeshTileStage", 35 * 35 + 4 * 72 * 72, mesh},
    };
    return all;
}

// argv: <res> <out.bin> stage <StageName|--list> [<in.f32>]
inline int main_stage(int argc, char **argv) {
    Run r;
    try {
        if (std::strcmp(argv[4], "--list") == 0) {
            for (const Scenario &s : scenarios()) std::printf("%s\n", s.name);
            return 0;
        }
        const Scenario *chosen = nullptr;
        for (const Scenario &s : scenarios())
            if (std::strcmp(argv[4], s.name) == 0) chosen = &s;
        if (!chosen) throw std::runtime_error(std::string("no stage scenario named ") + argv[4]);
        if (argc < 6) throw std::runtime_error("stage: no input file given");
        FILE *f = std::fopen(argv[5], "rb");
        if (!f) throw std::runtime_error(std::string("cannot open ") + argv[5]);
        r.in.resize(chosen->floats + 1);
        const size_t got = std::fread(r.in.data(), sizeof(float), r.in.size(), f);
        std::fclose(f);
        if (got != chosen->floats)
            throw std::runtime_error(std::string(chosen->name) + " reads " + std::to_string(chosen->floats) +
                                     " floats, the input file holds " + (got > chosen->floats ? "more" : std::to_string(got)));
        r.in.resize(chosen->floats);
        r.out = std::fopen(argv[2], "wb");
        if (!r.out) throw std::runtime_error(std::string("cannot open ") + argv[2]);
        check(nz_ctx_create(0, &r.ctx), "nz_ctx_create");
        chosen->run(r);
        if (r.at != r.in.size()) throw std::runtime_error("the scenario did not read all of its input");
        std::fclose(r.out);
        nz_ctx_destroy(r.ctx);
    } catch (const std::exception &e) {
        std::fflush(stdout);
        std::fprintf(stderr, "host_demo: %s\n", e.what());
        return 1;
    }
    return 0;
}

// ---- host_demo <res> <out.bin> sediment <in.f32>: SedimentFluvialStage, which schedules through ImplicitFluvialStage and so
// has no scenario of the `stage` table.  <in.f32>: the heights (res^2, behind a depression fill), rainMap, hardness, upliftMap
// (res^2 each), then for the res - 1 = 3 * m corner of the heights that corner and its nine m^2 blocks, block by block.
// a: defaults at dt 50, 3 iterations; b: every option -- erodibility .1, uplift .01, dt 20, rain 2, a sea, the three maps, an
// ample budget, Multiple routing with exponent 2, deposition 1, sedimentIterations 2, recordFlux, 2 iterations; c: the defaults
// of a with recordFlux on a payload with a WRITE plane; d1, d: the corner, then its nine blocks as a batch of the same length;
// e: a budget of 2 at 2 iterations; f: OnDestroy().  Planes and values as in the `stage` mode.
inline void dump_sediment(Run &r, const std::string &s, SedimentFluvialStage &st) {
    dump_implicit(r, s, st);
    r.f32_or_null(s + ".flux", st.flux(), st.cells());
    const float res = st.residual();
    uint32_t word;
    std::memcpy(&word, &res, 4);
    r.value(s + ".residual_bits", (long)word);
}

inline void sediment(Run &r, int res) {
    const int m = (res - 1) / 3;
    const size_t n = (size_t)res * res, nc = (size_t)9 * m * m;
    const float *h = r.take(n), *maps[3] = {r.take(n), r.take(n), r.take(n)}, *corner = r.take(nc), *blocks = r.take(nc);
    SedimentFluvialStage st(r.ctx);
    Driver d({&st});
    auto through = [&](const std::string &step, const float *host, int rs, int count, bool pair = false) {
        auto p = payload(r, host, rs, count, pair);
        if (d.run(p->gd()) != p->gd()) throw std::runtime_error("the stage handed on another payload");
        r.f32(step + ".height", p->gd()->data->ptr, p->cells());
        dump_sediment(r, step, st);
        if (pair) r.value(step + ".swapped", p->gd()->data == p->second.get() && p->gd()->write == p->first.get());
    };
    st.dt = 50.f;
    st.iterations = 3;
    through("a", h, res, 1);
    std::unique_ptr<DeviceTile> t[3];
    for (int k = 0; k < 3; k++) t[k] = r.tile(maps[k], n);
    SedimentFluvialStage opt(r.ctx);
    Driver dopt({&opt});
    opt.iterations = 2;
    opt.erodibility = .1f;
    opt.uplift = .01f;
    opt.dt = 20.f;
    opt.rain = 2.f;
    opt.seaLevel = SEA;
    opt.maxPasses = AMPLE;
    opt.rainMap = t[0].get();
    opt.hardness = t[1].get();
    opt.upliftMap = t[2].get();
    opt.routing = FlowRouting::Multiple;
    opt.flowExponent = 2;
    opt.deposition = 1.f;
    opt.sedimentIterations = 2;
    opt.recordFlux = true;
    {
        auto p = payload(r, h, res, 1);
        dopt.run(p->gd());
        r.f32("b.height", p->gd()->data->ptr, p->cells());
        dump_sediment(r, "b", opt);
    }
    opt.OnDestroy();
    st.recordFlux = true;
    through("c", h, res, 1, true);
    st.recordFlux = false;
    st.iterations = 1;
    through("d1", corner, 3 * m, 1);
    through("d", blocks, m, 9);
    st.iterations = 2;
    st.maxPasses = 2;
    through("e", h, res, 1);
    st.OnDestroy();
    dump_sediment(r, "f", st);
}

// argv: <res> <out.bin> sediment <in.f32>
inline int main_sediment(int argc, char **argv) {
    Run r;
    try {
        const int res = std::atoi(argv[1]);
        if (res < 4 || res % 3 != 1) throw std::runtime_error("sediment: the resolution must be 3 m + 1, m >= 1");
        if (argc < 5) throw std::runtime_error("sediment: no input file given");
        const size_t floats = (size_t)4 * res * res + (size_t)2 * (res - 1) * (res - 1);
        FILE *f = std::fopen(argv[4], "rb");
        if (!f) throw std::runtime_error(std::string("cannot open ") + argv[4]);
        r.in.resize(floats + 1);
        const size_t got = std::fread(r.in.data(), sizeof(float), r.in.size(), f);
        std::fclose(f);
        if (got != floats) throw std::runtime_error("sediment reads " + std::to_string(floats) + " floats");
        r.in.resize(floats);
        r.out = std::fopen(argv[2], "wb");
        if (!r.out) throw std::runtime_error(std::string("cannot open ") + argv[2]);
        check(nz_ctx_create(0, &r.ctx), "nz_ctx_create");
        sediment(r, res);
        if (r.at != r.in.size()) throw std::runtime_error("the mode did not read all of its input");
        std::fclose(r.out);
        nz_ctx_destroy(r.ctx);
    } catch (const std::exception &e) {
        std::fflush(stdout);
        std::fprintf(stderr, "host_demo: %s\n", e.what());
        return 1;
    }
    return 0;
}
}  // namespace stage_demo
