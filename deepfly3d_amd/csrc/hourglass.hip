// a2: stacked-hourglass engine -- the C ABI (include/df3d_hip.h).  The engine itself: hg_plan.h (the plan: which kernel runs on which tensor,
// the parameter manifest, the workspace and the weight-stream layout), hg_weights.h (weight packing), hg_launch.h (the launches).
#include "hg_plan.h"
#include "hg_launch.h"
#include "hg_weights.h"
static_assert(hgk::WN_U2_BYTES <= hgk::BRF_STREAM_BYTES, "U's second part fits the identity block's stage-image slot");
static_assert(hgk::WN_U2_BYTES <= hgk::L2F_STREAM_BYTES, "layer2: U's second part fits the stage-image slot");

namespace {

int check_forward_args(df3d_hg* h, const void* images, int n, void* ws, size_t ws_bytes) {
    DF3D_CHECK_ARG(h != nullptr, "null handle");
    if (!h->blob) {
        df3d::set_error("df3d_hg_forward: weights not set (call df3d_hg_set_weights first)");
        return DF3D_ESTATE;
    }
    DF3D_CHECK_ARG(n > 0, "n must be positive");
    DF3D_CHECK_ARG(images && ws, "null pointer");
    DF3D_CHECK_ARG(ws_bytes >= df3d_hg_workspace_bytes(h, n), "workspace too small");
    DF3D_CHECK_ARG((reinterpret_cast<uintptr_t>(ws) & 255) == 0, "workspace must be 256-byte aligned");
    return DF3D_OK;
}

}  // namespace

extern "C" {

#ifdef DF3D_BT_TIMING
// development build only: read and clear the per-phase cycle sums of bottleneck_ring_kernel
int df3d_dbg_ring_cycles(unsigned long long* out8) {
    // (twelve counters since round 4: out8 must hold 12 values)
    if (hipMemcpyFromSymbol(out8, HIP_SYMBOL(hgk::br_dbg), 96) != hipSuccess) return -1;
    unsigned long long z[12] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
    return hipMemcpyToSymbol(HIP_SYMBOL(hgk::br_dbg), z, 96) == hipSuccess ? 0 : -1;
}
#endif

int df3d_hg_create(int dtype, int num_stacks, df3d_hg** out) {
    DF3D_CHECK_ARG(out != nullptr, "null out");
    DF3D_CHECK_ARG(dtype == DF3D_DTYPE_F32 || dtype == DF3D_DTYPE_BF16 || dtype == DF3D_DTYPE_F16 || dtype == DF3D_DTYPE_F32S, "dtype must be DF3D_DTYPE_F32, DF3D_DTYPE_BF16, DF3D_DTYPE_F16 or DF3D_DTYPE_F32S");
    DF3D_CHECK_ARG(num_stacks >= 1 && num_stacks <= 8, "num_stacks must be in [1, 8]");
    df3d_hg* h = new df3d_hg();
    h->dtype = dtype;
    h->num_stacks = num_stacks;
    h->build();
    *out = h;
    return DF3D_OK;
}

void df3d_hg_destroy(df3d_hg* h) {
    if (!h) return;
    for (auto& t : h->prof.timed) {
        (void)hipEventDestroy(t.a);
        (void)hipEventDestroy(t.b);
    }
    for (auto e : h->prof.event_pool) (void)hipEventDestroy(e);
    delete h;
}

int df3d_hg_set_input(df3d_hg* h, int height, int width) {
    DF3D_CHECK_ARG(h != nullptr, "null handle");
    DF3D_CHECK_ARG(height > 0 && width > 0 && height % 64 == 0 && width % 64 == 0, "input height and width must be multiples of 64");
    h->H = height;
    h->W = width;
    h->build();  // (the parameter manifest does not depend on the spatial size: weights that are set stay valid)
    return DF3D_OK;
}

int df3d_hg_set_option(df3d_hg* h, const char* key, int value) {
    struct Option {
        const char* key;
        int df3d_hg::*member;
        bool (*accepts)(int value);
        const char* bad_value;       // the refusal of a value `accepts` turns down
        bool replans;                // the plan depends on it: build() again
        const char* after_weights;   // the refusal once df3d_hg_set_weights has run (what was packed follows the plan); nullptr: settable any time
        bool on_off = false;         // the plan sees only whether the value is > 0: another value of the same kind neither re-plans nor is refused
    };
    constexpr auto bit = [](int v) { return v == 0 || v == 1; };
    static const Option options[] = {
        {"fuse", &df3d_hg::fuse, bit, "fuse must be 0 or 1", true, "set 'fuse' before df3d_hg_set_weights (it changes the parameter manifest)"},
        {"fuse_upadd", &df3d_hg::fuse_upadd, [](int v) { return v >= 0 && v <= 2; }, "fuse_upadd must be 0, 1 or 2", true,
         "set 'fuse_upadd' before df3d_hg_set_weights (it changes the plan)"},
        {"l1", &df3d_hg::l1, bit, "l1 must be 0 or 1", true, "set 'l1' before df3d_hg_set_weights (it changes the plan and the low-precision buffer)"},
        {"ring", &df3d_hg::ring, bit, "ring must be 0 or 1", true, "set 'ring' before df3d_hg_set_weights (it changes the low-precision buffer)"},
        {"w2d", &df3d_hg::w2d, bit, "w2d must be 0 or 1", true, "set 'w2d' before df3d_hg_set_weights (it changes the weight streams)"},
        {"ring2", &df3d_hg::ring2, bit, "ring2 must be 0 or 1", false, nullptr},
        {"split1", &df3d_hg::split1, [](int v) { return v == 0 || v == 1 || (v >= 8 && v < 16); },
         "split1 must be 0, 1 or 8 + a mask (1 identity blocks, 2 layer1, 4 layer2)", true,
         "set 'split1' before df3d_hg_set_weights (it changes the plan and the weight streams)"},
        {"wino", &df3d_hg::wino, bit, "wino must be 0 or 1", true, "set 'wino' before df3d_hg_set_weights (it changes the weight streams)"},
        {"c1res", &df3d_hg::c1res, bit, "c1res must be 0 or 1", false, nullptr},
        {"no_reuse", &df3d_hg::no_reuse, bit, "no_reuse must be 0 or 1", true, "set 'no_reuse' before df3d_hg_set_weights (it changes the workspace plan)"},
        {"chain_views", &df3d_hg::chain_views, [](int v) { return v >= 0; }, "chain_views must be >= 0", true,
         "switch 'chain_views' on or off before df3d_hg_set_weights (it changes the workspace plan)", true},
        {"row_bytes", &df3d_hg::rb_override, [](int v) { return v == 0 || v == 64 || v == 128; }, "row_bytes must be 0, 64 or 128", false, nullptr},
    };
    DF3D_CHECK_ARG(h && key, "null argument");
    for (const Option& o : options) {
        if (strcmp(key, o.key)) continue;
        DF3D_CHECK_ARG(o.accepts(value), o.bad_value);
        const bool replan = o.replans && (!o.on_off || (value > 0) != (h->*o.member > 0));
        DF3D_CHECK_ARG(!replan || h->blob == nullptr, o.after_weights);
        h->*o.member = value;
        if (replan) h->build();
        return DF3D_OK;
    }
    df3d::set_error("df3d_hg_set_option: unknown key %s", key);
    return DF3D_EINVAL;
}

int df3d_hg_num_params(const df3d_hg* h) { return h ? (int)h->params.size() : 0; }

int df3d_hg_param_desc(const df3d_hg* h, int i, df3d_hg_param* out) {
    DF3D_CHECK_ARG(h && out, "null argument");
    DF3D_CHECK_ARG(i >= 0 && i < (int)h->params.size(), "index out of range");
    *out = h->params[i];
    return DF3D_OK;
}

size_t df3d_hg_blob_floats(const df3d_hg* h) { return h ? h->blob_floats : 0; }

size_t df3d_hg_lowp_bytes(const df3d_hg* h) {
    if (!h) return 0;
    // bf16: bf16 copy of the blob + the pre-swizzled weight streams of the ring bottlenecks; f32: the weight streams only
    return h->stream_base() + h->stream_bytes;
}

int df3d_hg_set_weights(df3d_hg* h, const float* blob_dev, void* lowp_dev, void* stream) {
    return hg_weights::df3d_hg_set_weights(h, blob_dev, lowp_dev, df3d::as_stream(stream));
}

size_t df3d_hg_workspace_bytes(const df3d_hg* h, int n) {
    if (!h || n <= 0) return 0;
    return h->act_elems_per_view * (size_t)n * h->elem_bytes() + 256;
}

int df3d_hg_forward(df3d_hg* h, const float* images_dev, int n, float* heatmaps_dev, void* workspace_dev,
                    size_t workspace_bytes, void* stream) {
    if (int rc = check_forward_args(h, images_dev, n, workspace_dev, workspace_bytes)) return rc;
    DF3D_CHECK_ARG(heatmaps_dev != nullptr, "null heatmaps");
    unsigned char* act = reinterpret_cast<unsigned char*>(workspace_dev);
    return run_steps_dtype(h, images_dev, n, (int)h->steps.size(), heatmaps_dev, act, df3d::as_stream(stream));
}

int df3d_hg_forward_u8(df3d_hg* h, const unsigned char* frames_dev, const unsigned char* flip_dev, int n, int frame_h, int frame_w, int frame_c,
                       const float* mean3_host, const float* std3_host, int resize, float* heatmaps_dev, void* workspace_dev, size_t workspace_bytes,
                       void* stream) {
    if (int rc = check_forward_args(h, frames_dev, n, workspace_dev, workspace_bytes)) return rc;
    DF3D_CHECK_ARG(heatmaps_dev != nullptr && mean3_host && std3_host, "null pointer");
    DF3D_CHECK_ARG(frame_h > 0 && frame_w > 0 && (frame_c == 1 || frame_c == 3), "bad frame shape (C must be 1 or 3)");
    DF3D_CHECK_ARG(resize >= DF3D_RESIZE_BILINEAR && resize <= DF3D_RESIZE_AREA, "resize must be one of DF3D_RESIZE_*");
    hgk::StemU8 u;
    u.nm.resize = resize;
    u.frames = frames_dev;
    u.flip = flip_dev;
    u.FH = frame_h;
    u.FW = frame_w;
    u.FC = frame_c;
    for (int c = 0; c < 3; ++c) {
        DF3D_CHECK_ARG(std3_host[c] != 0.0f, "std must be non-zero");
        u.nm.mean[c] = mean3_host[c];
        u.nm.inv_std[c] = 1.0f / std3_host[c];
    }
    h->u8in = u;
    unsigned char* act = reinterpret_cast<unsigned char*>(workspace_dev);
    const int rc = run_steps_dtype(h, nullptr, n, (int)h->steps.size(), heatmaps_dev, act, df3d::as_stream(stream));
    h->u8in.frames = nullptr;
    return rc;
}

int df3d_hg_work(const df3d_hg* h, int n, double* flops, double* bytes) {
    DF3D_CHECK_ARG(h && flops && bytes, "null argument");
    *flops = h->flops_per_view * n;
    *bytes = h->elems_per_view * n * h->elem_bytes();
    return DF3D_OK;
}

int df3d_hg_profile(df3d_hg* h, int enable) {
    DF3D_CHECK_ARG(h != nullptr, "null handle");
    h->prof.profiling = enable != 0;
    for (auto& t : h->prof.timed) {
        h->prof.event_pool.push_back(t.a);
        h->prof.event_pool.push_back(t.b);
    }
    h->prof.timed.clear();
    return DF3D_OK;
}

int df3d_hg_profile_count(const df3d_hg* h) { return h ? (int)h->prof.kernel_names.size() : 0; }

int df3d_hg_profile_read(df3d_hg* h, int kernel_class, char* name_buf, int buflen, double* ms, double* flops, double* bytes, double* bytes_m1,
                         int* launches) {
    DF3D_CHECK_ARG(h && name_buf && buflen > 0 && ms && flops && bytes && bytes_m1 && launches, "null argument");
    DF3D_CHECK_ARG(kernel_class >= 0 && kernel_class < (int)h->prof.kernel_names.size(), "kernel_class out of range");
    snprintf(name_buf, buflen, "%s", h->prof.kernel_names[kernel_class].c_str());
    *ms = *flops = *bytes = *bytes_m1 = 0.0;
    *launches = 0;
    for (auto& t : h->prof.timed) {
        if (t.cls != kernel_class) continue;
        DF3D_HIP(hipEventSynchronize(t.b));
        float e = 0.f;
        DF3D_HIP(hipEventElapsedTime(&e, t.a, t.b));
        *ms += e;
        *flops += t.w.flops;
        *bytes += t.w.bytes;
        *bytes_m1 += t.w.bytes_m1;
        *launches += 1;
    }
    return DF3D_OK;
}

int df3d_hg_profile_executed_flops(df3d_hg* h, int kernel_class, double* flops_executed) {
    DF3D_CHECK_ARG(h && flops_executed, "null argument");
    DF3D_CHECK_ARG(kernel_class >= 0 && kernel_class < (int)h->prof.kernel_names.size(), "kernel_class out of range");
    *flops_executed = 0.0;
    for (auto& t : h->prof.timed)
        if (t.cls == kernel_class) *flops_executed += t.w.flops_executed;
    return DF3D_OK;
}

int df3d_hg_num_steps(const df3d_hg* h) { return h ? (int)h->steps.size() : 0; }

double df3d_hg_step_m1_bytes(const df3d_hg* h, int step, int n) {
    if (!h || step < 0 || step >= (int)h->steps.size() || n <= 0) return 0.0;
    return h->steps[step].m1_elems * n * h->elem_bytes();
}

int df3d_hg_step_desc(const df3d_hg* h, int step, char* name_buf, int buflen, int* hwc) {
    DF3D_CHECK_ARG(h && name_buf && hwc && buflen > 0, "null argument");
    DF3D_CHECK_ARG(step >= 0 && step < (int)h->steps.size(), "step out of range");
    const Step& st = h->steps[step];
    snprintf(name_buf, buflen, "%s", st.name.c_str());
    if (st.out >= 0) {
        const TensorDesc& t = h->tensors[st.out];
        hwc[0] = t.h;
        hwc[1] = t.w;
        hwc[2] = t.c;
    } else {
        hwc[0] = h->H / 4;
        hwc[1] = h->W / 4;
        hwc[2] = h->classes;
    }
    return DF3D_OK;
}

int df3d_hg_step_pooled(const df3d_hg* h, int step) {
    DF3D_CHECK_ARG(h, "null argument");
    DF3D_CHECK_ARG(step >= 0 && step < (int)h->steps.size(), "step out of range");
    const Step& st = h->steps[step];
    return (st.pool_out >= 0 ? 1 : 0) | (st.pool_in >= 0 ? 2 : 0);
}

int df3d_hg_forward_upto(df3d_hg* h, const float* images_dev, int n, int upto, float* out_dev, void* workspace_dev,
                         size_t workspace_bytes, void* stream) {
    if (int rc = check_forward_args(h, images_dev, n, workspace_dev, workspace_bytes)) return rc;
    DF3D_CHECK_ARG(upto >= 1 && upto <= (int)h->steps.size(), "upto out of range");
    DF3D_CHECK_ARG(out_dev != nullptr, "null output");
    const Step& st = h->steps[upto - 1];
    unsigned char* act = reinterpret_cast<unsigned char*>(workspace_dev);
    hipStream_t s = df3d::as_stream(stream);
    // a final NCHW step writes straight into out_dev (as heat-maps)
    if (int rc = run_steps_dtype(h, images_dev, n, upto, out_dev, act, s)) return rc;
    if (st.out < 0) return DF3D_OK;
    const TensorDesc& t = h->tensors[st.out];
    const long long pixels = (long long)n * t.h * t.w;
    const long long total = pixels * t.c;
    const void* src = act + t.off * (size_t)n * h->elem_bytes();
    with_elem_type(h->dtype, [&](auto e) {   // (f32s tensors are float32 tensors)
        hipLaunchKernelGGL((export_kernel<StorageT<decltype(e)>>), dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s, src, out_dev, pixels,
                           t.c, t.pitch);
    });
    DF3D_LAUNCH_CHECK();
    return DF3D_OK;
}

}  // extern "C"
