// a2: stacked-hourglass engine -- the launches: one function per step kind of the plan (hg_plan.h), and run_steps, which walks the plan.
#pragma once
#include "hg_plan.h"

namespace {

// compute units of the current device (persistent kernels launch one workgroup per CU)
inline int cu_count() {
    static int cached[64] = {0};
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64) return 256;
    if (cached[dev] == 0) {
        int n = 0;
        cached[dev] = hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev) == hipSuccess && n > 0 ? n : 256;
    }
    return cached[dev];
}

// hipFuncSetAttribute acts on the CURRENT device: remember per device (bit i of `mask`) where it has been applied
inline bool first_use_on_this_device(unsigned& mask) {
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev > 31) return true;
    const bool first = !(mask & (1u << dev));
    mask |= 1u << dev;
    return first;
}

hipEvent_t get_event(df3d_hg* h) {
    if (!h->prof.event_pool.empty()) {
        hipEvent_t e = h->prof.event_pool.back();
        h->prof.event_pool.pop_back();
        return e;
    }
    hipEvent_t e = nullptr;
    (void)hipEventCreate(&e);
    return e;
}

struct ScopedTimer {
    df3d_hg* h;
    hipStream_t s;
    HgProfile::Timed t;
    bool on;
    ScopedTimer(df3d_hg* h_, hipStream_t s_, const std::string& name, const Work& w) : h(h_), s(s_), on(h_->prof.profiling) {
        if (!on) return;
        t = {get_event(h), get_event(h), h->prof.kernel_class(name), w};
        if (w.flops_executed < 0.0) t.w.flops_executed = w.flops;
        (void)hipEventRecord(t.a, s);
    }
    ~ScopedTimer() {
        if (!on) return;
        (void)hipEventRecord(t.b, s);
        h->prof.timed.push_back(t);
    }
};

template <typename T> struct TypeName;
template <> struct TypeName<float> { static constexpr const char* value = "float"; };
template <> struct TypeName<__hip_bfloat16> { static constexpr const char* value = "__hip_bfloat16"; };
template <> struct TypeName<_Float16> { static constexpr const char* value = "_Float16"; };
template <> struct TypeName<F32S> { static constexpr const char* value = "hgk::F32S"; };
// the element type of the kernels that only move or compare float32 data (pools, upsample-add, export): F32S tensors ARE float32 tensors
template <typename T> using StorageT = std::conditional_t<std::is_same<T, F32S>::value, float, T>;

inline std::string targ(bool v) { return v ? "true" : "false"; }
inline std::string targ(int v) { return std::to_string(v); }
inline std::string targ(const char* v) { return v; }
// a kernel instantiation's name as rocprofv3 prints it (the key of the profile tables): kname("k", float_name, 64, true) = "k<float, 64, true>"
template <typename... A>
std::string kname(const char* kernel, A... args) {
    std::string s = kernel;
    const char* sep = "<";
    ((s += sep, s += targ(args), sep = ", "), ...);
    return sizeof...(A) ? s + ">" : s;
}

// One launch of KERNEL, timed under `name` when profiling.  A kernel with dynamic LDS gets its limit raised once per device (the first
// launch's lds_bytes).
template <auto KERNEL, typename... A>
int launch_kernel(df3d_hg* h, const std::string& name, const Work& w, dim3 grid, int threads, int lds_bytes, hipStream_t s, const A&... args) {
    ScopedTimer tm(h, s, name, w);
    static unsigned attr_done = 0;
    if (lds_bytes > 0 && first_use_on_this_device(attr_done))
        DF3D_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(KERNEL), hipFuncAttributeMaxDynamicSharedMemorySize, lds_bytes));
    hipLaunchKernelGGL(KERNEL, grid, dim3(threads), lds_bytes, s, args...);
    DF3D_LAUNCH_CHECK();
    return DF3D_OK;
}

template <typename T, int TAPS, int BN, int RB>
int launch_conv_t(df3d_hg* h, const ConvArgs& a, const Work& w, hipStream_t s) {
    const dim3 grid((unsigned)((a.M + BM - 1) / BM), (unsigned)(a.cout / BN));
    return launch_kernel<conv_mfma_kernel<T, TAPS, BN, RB>>(h, kname("conv_mfma_kernel", TypeName<T>::value, TAPS, BN, RB), w, grid, 256,
                                                            2 * (BM + BN) * (RB + 16), s, a);
}

template <typename T, int TAPS, int BN>
int launch_conv_rb(df3d_hg* h, const ConvArgs& a, int rb, const Work& w, hipStream_t s) {
    if (rb == 128) return launch_conv_t<T, TAPS, BN, 128>(h, a, w, s);
    return launch_conv_t<T, TAPS, BN, 64>(h, a, w, s);
}

template <typename T>
int launch_conv(df3d_hg* h, const ConvArgs& a, int taps, int rb, const Work& w, hipStream_t s) {
    int bn = (a.cout % 128 == 0) ? 128 : (a.cout % 64 == 0 ? 64 : 32);
    // a launch too small to fill the chip with 128-channel tiles (the 4 x 8 hourglass level: 224 workgroups for 896 views) takes
    // narrower ones: four times the workgroups, each with a quarter of the weights to pull -- the same K order per output, so the
    // same bits
    const long long wgs128 = ((a.M + BM - 1) / BM) * (a.cout / bn);
    if (bn == 128 && wgs128 < 2LL * cu_count()) bn = taps == 1 ? 32 : 64;
    if (taps == 1) {
        if (bn == 128) return launch_conv_rb<T, 1, 128>(h, a, rb, w, s);
        if (bn == 64) return launch_conv_rb<T, 1, 64>(h, a, rb, w, s);
        return launch_conv_rb<T, 1, 32>(h, a, rb, w, s);
    }
    if (bn == 128) return launch_conv_rb<T, 9, 128>(h, a, rb, w, s);
    if (bn == 64) return launch_conv_rb<T, 9, 64>(h, a, rb, w, s);
    df3d::set_error("3x3 convolution with cout %d unsupported", a.cout);
    return DF3D_EINVAL;
}

template <typename T, bool LAST>
int launch_head(df3d_hg* h, const HeadArgs& a, const Work& w, hipStream_t s) {
    return launch_kernel<head_kernel<T, LAST>>(h, kname("head_kernel", TypeName<T>::value, LAST), w, dim3((unsigned)((a.M + 127) / 128)), 256,
                                               HeadCfg<T, LAST>::LDS_BYTES, s, a);
}

// one fused-bottleneck launch: pixels of its views, the M1 bytes of its step, its 8 x 16 output tiles
struct BtLaunch {
    double px, m1;
    int tiles;
    bool pool_only;
};
// the block's work in the reference's terms: conv1 (when this kernel runs it), the 3x3 (taps3 = 9; fewer: the MFMA work a Winograd kernel
// executes), conv3, the skip convolution (DS)
inline double bt_flops(double px, int cin, int pl, bool conv1, bool ds, double taps3 = 9.0) {
    return 2.0 * px * ((conv1 ? (double)cin * pl : 0.0) + taps3 * pl * pl + 2.0 * pl * pl + (ds ? 2.0 * cin * pl : 0.0));
}
// the least a launch moves: its input, t1 (the tails of the split forms), its output (the pooled quarter only: pool_only)
inline double bt_bytes(double px, int eb, int cin, int pl, bool t1, bool pool_only) {
    return px * eb * (cin + (t1 ? pl : 0) + (pool_only ? 0.5 * pl : 2.0 * pl));
}

template <typename T, int CIN, int PL, bool DS, bool UP = false, bool ADD2 = false>
int launch_bottleneck_t(df3d_hg* h, const BottleneckArgs& a, const BtLaunch& b, hipStream_t s) {
    return launch_kernel<bottleneck_kernel<T, CIN, PL, DS, UP, ADD2>>(
        h, kname("bottleneck_kernel", TypeName<T>::value, CIN, PL, DS, UP, ADD2),
        Work{bt_flops(b.px, CIN, PL, true, DS), bt_bytes(b.px, sizeof(T), CIN, PL, false, false), b.m1}, dim3(b.tiles), 256,
        BtCfg<T, CIN, PL, DS>::LDS_BYTES, s, a);
}

// The three variants of an identity-skip block's kernels: UP = the input is in + nearest-upsample(in2), ADD2 = the output gets
// + nearest-upsample(add2), or neither.  f(up, add2) receives them as std::bool_constants.
template <typename F>
int with_up_add2(const void* in2, const void* add2, F&& f) {
    if (in2) return f(std::true_type{}, std::false_type{});
    if (add2) return f(std::false_type{}, std::true_type{});
    return f(std::false_type{}, std::false_type{});
}

template <typename T>
int launch_l1_lp(df3d_hg* h, const BtL1Args& a, const BtLaunch& b, hipStream_t s) {
    const int tiles = a.V * (a.H / L1_TH) * (a.W / BT_TW);
    return launch_kernel<bottleneck_l1_kernel<T>>(h, kname("bottleneck_l1_kernel", TypeName<T>::value),
                                                  Work{bt_flops(b.px, 64, 64, true, true), bt_bytes(b.px, sizeof(T), 64, 64, false, b.pool_only), b.m1},
                                                  dim3(std::min(tiles, cu_count())), L1_WAVES * 64, L1_LDS_BYTES, s, a);
}

// MODE (hg_bt_ring.h): 0 = all weights through the ring, 1 = W2D (round 3), 2 = W2D + the round-4 form (option `ring2`)
template <typename T, bool UP, int CIN, bool ADD2, int MODE>
int launch_ring_lp_(df3d_hg* h, const BtRingArgs& r, const BtLaunch& b, int lds_bytes, hipStream_t s) {
    return launch_kernel<bottleneck_ring_kernel<T, UP, CIN, ADD2, MODE>>(
        h, kname("bottleneck_ring_kernel", TypeName<T>::value, UP, CIN, ADD2, MODE),
        Work{bt_flops(b.px, CIN, 128, true, CIN == 128), bt_bytes(b.px, sizeof(T), CIN, 128, false, false), b.m1}, dim3(b.tiles), 256, lds_bytes, s, r);
}
template <typename T, bool UP, int CIN, bool ADD2 = false>
int launch_ring_lp(df3d_hg* h, const BtRingArgs& r, const BtLaunch& b, int lds_bytes, hipStream_t s) {
    return !r.w2d    ? launch_ring_lp_<T, UP, CIN, ADD2, 0>(h, r, b, lds_bytes, s)
           : h->ring2 ? launch_ring_lp_<T, UP, CIN, ADD2, 2>(h, r, b, lds_bytes, s)
                      : launch_ring_lp_<T, UP, CIN, ADD2, 1>(h, r, b, lds_bytes, s);
}

// TAIL: the split form's tail (conv1 ran before, t1 comes from memory)
template <typename T, bool UP, bool ADD2, bool TAIL>
int launch_ring_f32(df3d_hg* h, const BtRingArgs& r, const BtLaunch& b, int lds_bytes, hipStream_t s) {
    return launch_kernel<bottleneck_ring_f32_kernel<UP, ADD2, TAIL, T>>(
        h, kname("bottleneck_ring_f32_kernel", UP, ADD2, TAIL, TypeName<T>::value),
        Work{bt_flops(b.px, 256, 128, !TAIL, false), bt_bytes(b.px, 4, 256, 128, TAIL, false), b.m1}, dim3(b.tiles), 256, lds_bytes, s, r);
}

// the ring kernels' dynamic LDS (development builds: more, to hold one workgroup per CU: > 80 KB)
inline int ring_lds_bytes() {
    int lds_bytes = BR_LDS_BYTES;
#ifdef DF3D_BT_TIMING
    if (const char* e = getenv("BR_LDS")) lds_bytes = atoi(e);
#endif
#ifdef BR_FORCE_LDS
    lds_bytes = BR_FORCE_LDS;
#endif
    return lds_bytes;
}

// conv1 of the split forms (hg_c1_f32.h): persistent, two workgroups per CU
template <typename T, bool UP, int CIN, int PL>
int launch_conv1_f32(df3d_hg* h, const Conv1Args& c, const BtLaunch& b, hipStream_t s) {
    return launch_kernel<conv1_ring_f32_kernel<UP, CIN, PL, T>>(h, kname("conv1_ring_f32_kernel", UP, CIN, PL, TypeName<T>::value),
                                                                Work{2.0 * b.px * CIN * PL, b.px * 4.0 * (CIN + PL), 0.0},
                                                                dim3((unsigned)std::min<long long>(c.M / 128, 2LL * cu_count())), 256, C1_LDS_BYTES, s, c);
}

// conv1 of the Winograd identity form with W1 resident in LDS (hg_c1_res_f32.h, option c1res): one workgroup per CU
inline int launch_conv1_res_f32(df3d_hg* h, const Conv1Args& c, const BtLaunch& b, hipStream_t s) {
    return launch_kernel<conv1_res_f32_kernel>(h, kname("conv1_res_f32_kernel"), Work{2.0 * b.px * 256 * 128, b.px * 4.0 * (256 + 128), 0.0},
                                               dim3((unsigned)std::min<long long>(c.M / 128, (long long)(cu_count() & ~7))), 256, C1R_LDS_BYTES, s, c);
}

template <typename T>
int launch_layer1_tail_f32(df3d_hg* h, const BtRingArgs& r, const BtLaunch& b, hipStream_t s) {
    return launch_kernel<layer1_tail_f32_kernel<T>>(h, kname("layer1_tail_f32_kernel", TypeName<T>::value),
                                                    Work{bt_flops(b.px, 64, 64, false, true), bt_bytes(b.px, 4, 64, 64, true, b.pool_only), b.m1},
                                                    dim3(b.tiles), 256, L1F_LDS_BYTES, s, r);
}

template <typename T>
int launch_layer2_tail_f32(df3d_hg* h, const BtRingArgs& r, const BtLaunch& b, hipStream_t s) {
    return launch_kernel<layer2_tail_f32_kernel<T>>(h, kname("layer2_tail_f32_kernel", TypeName<T>::value),
                                                    Work{bt_flops(b.px, 128, 128, false, true), bt_bytes(b.px, 4, 128, 128, true, false), b.m1},
                                                    dim3(b.tiles), 256, L2F_LDS_BYTES, s, r);
}

// The Winograd tails are persistent: one workgroup per CU (it needs the whole register file), walking tiles with stride gridDim; a
// multiple of 8 keeps virtual block ids on their XCD (hg_bt_wino_f32.h tile_of).  FLOPs: the direct form's; the kernels EXECUTE 24/72
// (F(2x4, 3x3)) or 4/9 (layer1's F(2x2, 3x3)) of the 3x3's.
template <bool UP, bool ADD2, bool L2>
int launch_wino_f32(df3d_hg* h, const BtRingArgs& r, const BtLaunch& b, hipStream_t s) {
    constexpr int CIN = L2 ? 128 : 256;
    const int cus = cu_count() & ~7;
    return launch_kernel<bottleneck_wino_f32_kernel<UP, ADD2, L2>>(
        h, kname("bottleneck_wino_f32_kernel", UP, ADD2, L2),
        Work{bt_flops(b.px, CIN, 128, false, L2), bt_bytes(b.px, 4, CIN, 128, true, false), b.m1, bt_flops(b.px, CIN, 128, false, L2, 3.0)},
        dim3(b.tiles <= cus ? b.tiles : cus), 256, WN_LDS_BYTES, s, r);
}

inline int launch_layer1_wino_f32(df3d_hg* h, const BtRingArgs& r, const BtLaunch& b, hipStream_t s) {
    const int tiles = r.V * (r.H / BT_TH) * (r.W / L1W_TW), cus = cu_count() & ~7;
    return launch_kernel<layer1_wino_f32_kernel>(
        h, kname("layer1_wino_f32_kernel"),
        Work{bt_flops(b.px, 64, 64, false, true), bt_bytes(b.px, 4, 64, 64, true, b.pool_only), b.m1, bt_flops(b.px, 64, 64, false, true, 4.0)},
        dim3(tiles <= cus ? tiles : cus), 256, L1W_LDS_BYTES, s, r);
}

// One plan step on the views [v0, v0 + n) of a batch of n_all: every tensor is [views][h][w][pitch], so a view range is a contiguous
// slice of each (the whole batch: v0 = 0, n = n_all).  T: the engine's element type.
template <typename T>
struct StepRun {
    static constexpr int eb = sizeof(T);
    df3d_hg* h;
    const float* images;    // of view v0 (nullptr: df3d_hg_forward_u8)
    float* heatmaps;        // of view v0
    unsigned char* act;
    int n_all, v0, n;
    hipStream_t s;
    // the weights the kernels read: the caller's float32 blob (f32), its 16-bit copy (bf16 / f16), its pre-split copy (f32s); biases and
    // BatchNorm coefficients always come from the blob
    const unsigned char* weights(size_t off) const {
        return reinterpret_cast<const unsigned char*>(std::is_same<T, float>::value ? (const void*)h->blob : h->lowp) + off * eb;
    }
    const unsigned char* wstream(long long off) const { return reinterpret_cast<const unsigned char*>(h->lowp) + h->stream_base() + off; }
    unsigned char* tptr(int id) const {
        if (id < 0) return nullptr;
        const TensorDesc& t = h->tensors[id];
        return act + (t.off * (size_t)n_all + (size_t)v0 * t.h * t.w * t.pitch) * eb;
    }
    double m1(const Step& st) const { return st.m1_elems * n * eb; }
};

template <typename T>
int launch_stem_step(const StepRun<T>& c, const Step& st) {
    constexpr int eb = sizeof(T);
    df3d_hg* const h = c.h;
    StemArgs a;
    a.img = c.images;
    a.out = c.tptr(st.out);
    a.w = h->blob + st.conv.w_off;
    // 16-bit: the [64][184] tile; f32s: the hi / lo half tiles in the stem's slot of the pre-split copy (stem_relayout_f32s_kernel)
    a.w_lp = std::is_same<T, float>::value ? nullptr : c.weights(st.conv.w_off);
    a.bias = h->blob + st.conv.b_off;
    a.V = c.n;
    a.H = h->H;
    a.W = h->W;
    a.u8 = h->u8in;
    if (a.u8.frames) {
        a.u8.frames += (size_t)c.v0 * a.u8.FH * a.u8.FW * a.u8.FC;
        if (a.u8.flip) a.u8.flip += c.v0;
    }
    const int blocks = c.n * (h->H / 2 / STEM_TH) * (h->W / 2 / STEM_TW);
    const double opx = (double)c.n * (h->H / 2) * (h->W / 2);
    const Work w{2.0 * opx * 147 * 64, opx * (12.0 * 4 + 64.0 * eb), c.m1(st)};
    // persistent: the weights once per workgroup; as many workgroups per CU as each kernel's LDS lets it hold (hg_stem.h)
    if constexpr (eb == 2) {
        return launch_kernel<stem_lp_kernel<T>>(h, kname("stem_lp_kernel", TypeName<T>::value), w, dim3(std::min(blocks, STEM_LP_WGS_PER_CU * cu_count())), 256, 0, c.s, a);
    } else if constexpr (std::is_same<T, F32S>::value) {
        return launch_kernel<stem_f32s_kernel>(h, kname("stem_f32s_kernel"), w, dim3(std::min(blocks, STEM_F32S_WGS_PER_CU * cu_count())), 256, 0, c.s, a);
    } else {
        return launch_kernel<stem_kernel<T>>(h, kname("stem_kernel", TypeName<T>::value), w, dim3(std::min(blocks, STEM_F32_WGS_PER_CU * cu_count())), 256, 0, c.s, a);
    }
}

template <typename T>
int launch_conv_step(const StepRun<T>& c, const Step& st) {
    constexpr int eb = sizeof(T);
    df3d_hg* const h = c.h;
    const TensorDesc& ti = h->tensors[st.in];
    ConvArgs a;
    a.in = c.tptr(st.in);
    a.out = c.tptr(st.out);
    a.res = c.tptr(st.res);
    a.out_nchw = st.conv.nchw_out ? c.heatmaps : nullptr;
    a.w = c.weights(st.conv.w_off);
    a.bias = h->blob + st.conv.b_off;
    a.scale = st.conv.preact ? h->blob + st.conv.s_off : nullptr;
    a.shift = st.conv.preact ? h->blob + st.conv.t_off : nullptr;
    a.M = (long long)c.n * ti.h * ti.w;
    a.H = ti.h;
    a.W = ti.w;
    a.cin = st.conv.cin_pad;
    a.cout = st.conv.cout_pad;
    a.in_pitch = ti.pitch;
    a.out_pitch = st.out >= 0 ? h->tensors[st.out].pitch : 0;
    a.res_pitch = st.res >= 0 ? h->tensors[st.res].pitch : 0;
    a.relu = st.conv.relu;
    a.cout_real = st.conv.cout;
    const int ke128 = 128 / eb;
    int rb = (st.conv.cin_pad % ke128 == 0) ? 128 : 64;
    if (h->rb_override == 64) rb = 64;
    const double mm = (double)a.M;
    const Work w{2.0 * mm * st.conv.taps * st.conv.cin * st.conv.cout, mm * eb * (st.conv.cin + st.conv.cout + (st.res >= 0 ? st.conv.cout : 0)), c.m1(st)};
    return launch_conv<T>(h, a, st.conv.taps, rb, w, c.s);
}

// what BottleneckArgs and BtL1Args have in common with BtRingArgs: the block's tensors, biases, bn1 coefficients and shape
template <typename A>
void copy_block_args(A& a, const BtRingArgs& r) {
    a.in = r.in; a.out = r.out; a.pool = r.pool;
    a.b1 = r.b1; a.b2 = r.b2; a.b3 = r.b3; a.bd = r.bd; a.s1 = r.s1; a.t1 = r.t1;
    a.V = r.V; a.H = r.H; a.W = r.W;
}

// An ST_BOTTLENECK step as the kernels of its form (BtForm, hg_plan.h): the weight streams each case passes are the ones the plan took
// for the form and set_weights packed (hg_weights.h pack_streams).
template <typename T>
int launch_bottleneck_step(const StepRun<T>& c, const Step& st) {
    constexpr int eb = sizeof(T);
    constexpr bool F32 = std::is_same<T, float>::value;
    df3d_hg* const h = c.h;
    hipStream_t const s = c.s;
    const TensorDesc& ti = h->tensors[st.in];
    const bool ds = st.res < 0;
    const int cin = st.conv.cin, pl = st.conv.cout, n = c.n;
    const BtLaunch b{(double)n * ti.h * ti.w, c.m1(st), n * (ti.h / BT_TH) * (ti.w / BT_TW), st.pool_only};
    // the block's tensors and biases, as every ring and tail kernel takes them; each form adds its weight streams
    BtRingArgs r{};
    r.in = c.tptr(st.in);
    r.in2 = c.tptr(st.in2);
    r.add2 = c.tptr(st.add2);
    r.out = st.pool_only ? nullptr : c.tptr(st.out);
    r.pool = st.pool_only ? c.tptr(st.out) : c.tptr(st.pool_out);
    r.pool_in = c.tptr(st.pool_in);
    r.b1 = h->blob + st.conv.b_off;
    r.b2 = h->blob + st.conv2b.b_off;
    r.b3 = h->blob + st.conv3b.b_off;
    r.bd = ds ? h->blob + st.conv4b.b_off : nullptr;
    r.s1 = h->blob + st.conv.s_off;
    r.t1 = h->blob + st.conv.t_off;
    r.V = n;
    r.H = ti.h;
    r.W = ti.w;
    // the split forms: conv1 writes t1 for every pixel of the level, the tail reads it (and the zero page: the 3x3's padding)
    Conv1Args c1{};
    if (st.t1 >= 0) {
        c1.in = r.in;
        c1.in2 = r.in2;
        c1.H = ti.h;
        c1.W = ti.w;
        c1.t1 = c.tptr(st.t1);
        c1.wstream = c.wstream(st.wstream_c1);
        c1.b1 = r.b1;
        c1.s1 = r.s1;
        c1.t1c = r.t1;
        c1.M = (long long)n * ti.h * ti.w;
        r.t1in = c1.t1;
        r.zeros = c.wstream(h->zero_off);
        if (c1.M % 128) {
            df3d::set_error("conv1 of the split bottleneck needs whole 128-pixel tiles (M = %lld)", c1.M);
            return DF3D_EINVAL;
        }
    }
    switch (st.form) {
        case BT_REG: {
            BottleneckArgs a;
            copy_block_args(a, r);
            a.in2 = r.in2;
            a.add2 = r.add2;
            a.w1 = c.weights(st.conv.w_off);
            a.w2 = c.weights(st.conv2b.w_off);
            a.w3 = c.weights(st.conv3b.w_off);
            a.wd = ds ? c.weights(st.conv4b.w_off) : nullptr;
            if (cin == 256 && pl == 128)
                return with_up_add2(a.in2, a.add2, [&](auto up, auto add2) { return launch_bottleneck_t<T, 256, 128, false, up.value, add2.value>(h, a, b, s); });
            if (cin == 128 && pl == 128) return launch_bottleneck_t<T, 128, 128, true>(h, a, b, s);
            if (cin == 64 && pl == 64) return launch_bottleneck_t<T, 64, 64, true>(h, a, b, s);
            df3d::set_error("fused bottleneck %d -> %d unsupported", cin, pl);
            return DF3D_EINVAL;
        }
        case BT_L1_LP:
            if constexpr (eb == 2) {
                BtL1Args a;
                copy_block_args(a, r);
                a.wimage = c.wstream(st.wstream);
                return launch_l1_lp<T>(h, a, b, s);
            }
            break;
        case BT_RING_LP:
            if constexpr (eb == 2) {
                r.wstream = c.wstream(st.wstream);
                r.w2d = st.wstream_w2 >= 0 ? c.wstream(st.wstream_w2) : nullptr;
                if (cin == 128) return launch_ring_lp<T, false, 128>(h, r, b, BR_LDS_BYTES, s);   // layer2
                return with_up_add2(r.in2, r.add2, [&](auto up, auto add2) { return launch_ring_lp<T, up.value, 256, add2.value>(h, r, b, ring_lds_bytes(), s); });
            }
            break;
        case BT_RING_F32:
            if constexpr (eb == 4) {
                r.wstream = c.wstream(st.wstream);
                return with_up_add2(r.in2, r.add2, [&](auto up, auto add2) { return launch_ring_f32<T, up.value, add2.value, false>(h, r, b, ring_lds_bytes(), s); });
            }
            break;
        case BT_SPLIT_F32:
            if constexpr (eb == 4) {
                if (int rc = r.in2 ? launch_conv1_f32<T, true, 256, 128>(h, c1, b, s) : launch_conv1_f32<T, false, 256, 128>(h, c1, b, s)) return rc;
                r.wstream = c.wstream(st.wstream);
                return with_up_add2(r.in2, r.add2, [&](auto up, auto add2) { return launch_ring_f32<T, up.value, add2.value, true>(h, r, b, ring_lds_bytes(), s); });
            }
            break;
        case BT_SPLIT_WINO:
            if constexpr (F32) {
                const bool resident = !r.in2 && h->c1res;
                if (resident) c1.wstream = c.wstream(st.wstream_wino + WN_STREAM_BYTES);   // W1, behind U's first part and W3'
                if (int rc = resident   ? launch_conv1_res_f32(h, c1, b, s)
                             : r.in2 ? launch_conv1_f32<T, true, 256, 128>(h, c1, b, s)
                                     : launch_conv1_f32<T, false, 256, 128>(h, c1, b, s))
                    return rc;
                r.w2d = c.wstream(st.wstream_wino);
                r.wstream = c.wstream(st.wstream_u2);
                return with_up_add2(r.in2, r.add2, [&](auto up, auto add2) { return launch_wino_f32<up.value, add2.value, false>(h, r, b, s); });
            }
            break;
        case BT_L1F:
            if constexpr (eb == 4) {
                if (int rc = launch_conv1_f32<T, false, 64, 64>(h, c1, b, s)) return rc;
                r.wstream = c.wstream(st.wstream);
                return launch_layer1_tail_f32<T>(h, r, b, s);
            }
            break;
        case BT_L1F_WINO:
            if constexpr (F32) {
                if (int rc = launch_conv1_f32<T, false, 64, 64>(h, c1, b, s)) return rc;
                r.w2d = c.wstream(st.wstream_wino);
                return launch_layer1_wino_f32(h, r, b, s);
            }
            break;
        case BT_L2F:
            if constexpr (eb == 4) {
                if (int rc = launch_conv1_f32<T, false, 128, 128>(h, c1, b, s)) return rc;
                r.wstream = c.wstream(st.wstream);
                return launch_layer2_tail_f32<T>(h, r, b, s);
            }
            break;
        case BT_L2F_WINO:
            if constexpr (F32) {
                if (int rc = launch_conv1_f32<T, false, 128, 128>(h, c1, b, s)) return rc;
                r.w2d = c.wstream(st.wstream_wino);
                r.wstream = c.wstream(st.wstream_u2);
                return launch_wino_f32<false, false, true>(h, r, b, s);
            }
            break;
    }
    df3d::set_error("bottleneck form %d has no kernels for this element type", (int)st.form);
    return DF3D_EINVAL;
}

template <typename T>
int launch_head_step(const StepRun<T>& c, const Step& st) {
    constexpr int eb = sizeof(T);
    df3d_hg* const h = c.h;
    const TensorDesc& ti = h->tensors[st.in];
    HeadArgs a;
    a.r = c.tptr(st.in);
    a.x = st.last ? nullptr : c.tptr(st.res);
    a.out = st.last ? nullptr : c.tptr(st.out);
    a.heat = st.last ? c.heatmaps : nullptr;
    a.wfc = c.weights(st.conv.w_off);
    a.wsc = c.weights(st.conv2b.w_off);
    a.bfc = h->blob + st.conv.b_off;
    a.bsc = h->blob + st.conv2b.b_off;
    a.wfc_ = st.last ? nullptr : c.weights(st.conv3b.w_off);
    a.wsc_ = st.last ? nullptr : c.weights(st.conv4b.w_off);
    a.bfc_ = st.last ? nullptr : h->blob + st.conv3b.b_off;
    a.bsc_ = st.last ? nullptr : h->blob + st.conv4b.b_off;
    a.M = (long long)c.n * ti.h * ti.w;
    a.HW = ti.h * ti.w;
    a.fcstream = st.wstream >= 0 ? c.wstream(st.wstream) : nullptr;
    a.fc2stream = st.wstream2 >= 0 && a.M % 128 == 0 ? c.wstream(st.wstream2) : nullptr;
    const double mm = (double)a.M;
    const double fl = 2.0 * mm * (256.0 * 256 + 256.0 * 19 + (st.last ? 0.0 : 256.0 * 256 + 19.0 * 256));
    const Work w{fl, mm * eb * (st.last ? 256.0 : 768.0) + (st.last ? mm * 19 * 4 : 0.0), c.m1(st)};
    return st.last ? launch_head<T, true>(h, a, w, c.s) : launch_head<T, false>(h, a, w, c.s);
}

template <typename T>
int launch_pool_step(const StepRun<T>& c, const Step& st) {
    const TensorDesc& to = c.h->tensors[st.out];
    const int chunks = to.pitch * c.eb / 16;
    const long long total = (long long)c.n * to.h * to.w * chunks;
    return launch_kernel<pool2_kernel<StorageT<T>>>(c.h, kname("pool2_kernel", TypeName<StorageT<T>>::value), Work{0.0, (double)total * 16 * 5, c.m1(st)},
                                                    dim3((unsigned)((total + 255) / 256)), 256, 0, c.s, reinterpret_cast<const u32x4*>(c.tptr(st.in)),
                                                    reinterpret_cast<u32x4*>(c.tptr(st.out)), total, to.h, to.w, chunks);
}

template <typename T>
int launch_upadd_step(const StepRun<T>& c, const Step& st) {
    const TensorDesc& to = c.h->tensors[st.out];
    const int chunks = to.pitch * c.eb / 16;
    const long long total = (long long)c.n * to.h * to.w * chunks;
    return launch_kernel<upadd_kernel<StorageT<T>>>(c.h, kname("upadd_kernel", TypeName<StorageT<T>>::value), Work{0.0, (double)total * 16 * 2.25, c.m1(st)},
                                                    dim3((unsigned)((total + 255) / 256)), 256, 0, c.s, reinterpret_cast<const u32x4*>(c.tptr(st.in)),
                                                    reinterpret_cast<const u32x4*>(c.tptr(st.res)), reinterpret_cast<u32x4*>(c.tptr(st.out)), total, to.h,
                                                    to.w, chunks);
}

template <typename T>
int run_steps(df3d_hg* h, const float* images_all, int n_all, int upto, float* heatmaps_all, unsigned char* act, hipStream_t s) {
    auto launch = [&](int i, int v0, int n) -> int {
        const StepRun<T> c{h, images_all ? images_all + (size_t)v0 * h->H * h->W * 3 : nullptr,
                           heatmaps_all ? heatmaps_all + (size_t)v0 * h->classes * (h->H / 4) * (h->W / 4) : nullptr, act, n_all, v0, n, s};
        const Step& st = h->steps[i];
        switch (st.kind) {
            case ST_STEM: return launch_stem_step(c, st);
            case ST_CONV: return launch_conv_step(c, st);
            case ST_BOTTLENECK: return launch_bottleneck_step(c, st);
            case ST_HEAD: return launch_head_step(c, st);
            case ST_POOL: return launch_pool_step(c, st);
            case ST_UPADD: return launch_upadd_step(c, st);
        }
        return DF3D_OK;
    };
    // Chains: runs of consecutive full-resolution steps are walked in chunks of `chain_views` views, so that what one step
    // writes is still in the 256 MB Infinity Cache when the next one reads it (a whole 896-view batch moves 3.8 GB per
    // tensor: nothing survives from one launch to the next).  The steps of a chain only read tensors of their own view range.
    for (int i = 0; i < upto;) {
        int j = i + 1;
        const int cv = h->chain_views;
        if (cv > 0 && cv < n_all && h->chain_end[i] > i + 1) {
            j = std::min(h->chain_end[i], upto);
            for (int v0 = 0; v0 < n_all; v0 += cv)
                for (int k = i; k < j; ++k)
                    if (int rc = launch(k, v0, std::min(cv, n_all - v0))) return rc;
        } else if (int rc = launch(i, 0, n_all)) {
            return rc;
        }
        i = j;
    }
    return DF3D_OK;
}

// f(T{}) with the element type T of engine dtype `dtype` (DF3D_DTYPE_*)
template <typename F>
auto with_elem_type(int dtype, F&& f) {
    switch (dtype) {
        case DF3D_DTYPE_F32: return f(float{});
        case DF3D_DTYPE_F32S: return f(F32S{});
        case DF3D_DTYPE_F16: return f(_Float16{});
        default: return f(__hip_bfloat16{});
    }
}

int run_steps_dtype(df3d_hg* h, const float* images, int n, int upto, float* heatmaps, unsigned char* act, hipStream_t s) {
    return with_elem_type(h->dtype, [&](auto t) { return run_steps<decltype(t)>(h, images, n, upto, heatmaps, act, s); });
}

}  // namespace
