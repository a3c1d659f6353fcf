// a2: stacked-hourglass engine -- weight packing: the 16-bit / pre-split copy of the blob and the weight streams the plan (hg_plan.h) laid out.
#pragma once
#include "hg_launch.h"

extern "C" {   // (the kernel's symbol stays plain `absmax_bits_kernel`)
namespace {
// max |w| over the blob as an integer (the bit pattern of |x| orders like the value; an infinity or a NaN is >= 0x7f800000)
__global__ __launch_bounds__(256) void absmax_bits_kernel(const float* __restrict__ w, size_t n, unsigned* __restrict__ out) {
    unsigned m = 0;
    for (size_t i = blockIdx.x * (size_t)256 + threadIdx.x; i < n; i += (size_t)gridDim.x * 256) m = max(m, __float_as_uint(w[i]) & 0x7fffffffu);
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) m = max(m, (unsigned)__shfl_xor((int)m, off, 64));
    if ((threadIdx.x & 63) == 0) atomicMax(out, m);
}
}  // namespace
}  // extern "C"

namespace {

// The stream packers move one 16-byte chunk per thread
inline dim3 pack_grid(size_t stream_bytes) { return dim3((unsigned)((stream_bytes / 16 + 255) / 256)); }

// The weight streams behind stream_base(): what each step's kernels read besides the blob, slot by slot as the plan took them (hg_plan.h,
// bottleneck()) and as launch_bottleneck_step passes them on (hg_launch.h).  The 16-bit forms pack from the 16-bit copy of the blob at the
// start of the buffer, the others from `w` (the float32 blob; f32s: its pre-split copy).
int pack_streams(df3d_hg* h, void* lowp_dev, const float* w, hipStream_t s) {
    const unsigned short* const lp = reinterpret_cast<const unsigned short*>(lowp_dev);
    unsigned char* const base = reinterpret_cast<unsigned char*>(lowp_dev) + h->stream_base();
    auto floats = [&](long long off) { return reinterpret_cast<float*>(base + off); };
    for (const Step& st : h->steps) {
        if (st.kind == ST_HEAD && st.wstream >= 0) {
            if (!h->lp()) {
                hipLaunchKernelGGL(bt_fc_pack_f32_kernel, pack_grid(HD_FC_STREAM_BYTES_F32), dim3(256), 0, s, w + st.conv.w_off, base + st.wstream);
                continue;
            }
            hipLaunchKernelGGL(bt_fc_pack_kernel, pack_grid(HD_FC_STREAM_BYTES), dim3(256), 0, s, lp + st.conv.w_off, base + st.wstream);
            if (st.wstream2 >= 0)
                hipLaunchKernelGGL(bt_fc2_pack_kernel, pack_grid(HD_FC2_STREAM_BYTES), dim3(256), 0, s, lp + st.conv3b.w_off, lp + st.conv4b.w_off,
                                   base + st.wstream2);
            continue;
        }
        if (st.kind != ST_BOTTLENECK) continue;
        const long long w1 = st.conv.w_off, w2 = st.conv2b.w_off, w3 = st.conv3b.w_off, wd = st.conv4b.w_off;
        const int cin = st.conv.cin, pl = st.conv.cout;
        // conv1's stage images of the split forms
        auto pack_c1 = [&] { hipLaunchKernelGGL(bt_c1_pack_f32_kernel, pack_grid(c1_stream_bytes(cin)), dim3(256), 0, s, w + w1, base + st.wstream_c1, cin, pl); };
        // U of bottleneck_wino_f32_kernel (its first part in the Winograd slot, its second in wstream_u2: no launch of a Winograd form reads
        // direct-form stage images) and, behind the first part, the permuted rows of W3
        auto pack_wino = [&] {
            hipLaunchKernelGGL(bt_wino_pack_kernel, dim3(128 * 128 / 256), dim3(256), 0, s, w + w2, floats(st.wstream_wino), floats(st.wstream_u2));
            hipLaunchKernelGGL(bt_wino_pack_w3_kernel, pack_grid(WN_W3_BYTES), dim3(256), 0, s, w + w3, base + st.wstream_wino + WN_U_BYTES);
        };
        switch (st.form) {
            case BT_REG: break;
            case BT_L1_LP:
                hipLaunchKernelGGL(bt_l1_pack_kernel, pack_grid(L1_W_BYTES), dim3(256), 0, s, lp + w1, lp + w2, lp + w3, lp + wd, base + st.wstream);
                break;
            case BT_RING_LP: {
                if (st.wstream_w2 >= 0) hipLaunchKernelGGL(bt_w2d_pack_kernel, pack_grid(BR_W2D_BYTES), dim3(256), 0, s, lp + w2, base + st.wstream_w2);
                const bool ds = st.res < 0;   // layer2: 128 -> 128 -> 128 -> 256 with the skip convolution
                hipLaunchKernelGGL(bt_ring_pack_kernel, pack_grid(br_stream_bytes(cin, ds)), dim3(256), 0, s, lp + w1, lp + w2, lp + w3, ds ? lp + wd : nullptr,
                                   cin, base + st.wstream);
                break;
            }
            case BT_RING_F32:
            case BT_SPLIT_F32:
                hipLaunchKernelGGL(bt_ring_pack_f32_kernel, pack_grid(BRF_STREAM_BYTES), dim3(256), 0, s, w + w1, w + w2, w + w3, base + st.wstream);
                if (st.form == BT_SPLIT_F32) pack_c1();
                break;
            case BT_SPLIT_WINO:
                pack_c1();
                pack_wino();
                hipLaunchKernelGGL(c1r_pack_kernel, pack_grid(C1R_W_BYTES), dim3(256), 0, s, w + w1, base + st.wstream_wino + WN_STREAM_BYTES);
                break;
            case BT_L1F:
                hipLaunchKernelGGL(bt_l1f_pack_kernel, pack_grid(L1F_STREAM_BYTES), dim3(256), 0, s, w + w2, w + w3, w + wd, base + st.wstream);
                pack_c1();
                break;
            case BT_L1F_WINO:   // (nothing goes into the slot of L1F_WINO_UNUSED_SLOT_BYTES)
                pack_c1();
                hipLaunchKernelGGL(l1_wino_pack_u_kernel, dim3(64 * 64 / 256), dim3(256), 0, s, w + w2, floats(st.wstream_wino));
                hipLaunchKernelGGL(l1_wino_pack_w_kernel, pack_grid(L1W_W_BYTES), dim3(256), 0, s, w + w3, base + st.wstream_wino + L1W_U_BYTES);
                hipLaunchKernelGGL(l1_wino_pack_w_kernel, pack_grid(L1W_W_BYTES), dim3(256), 0, s, w + wd, base + st.wstream_wino + L1W_U_BYTES + L1W_W_BYTES);
                break;
            case BT_L2F:
                hipLaunchKernelGGL(bt_l2f_pack_kernel, pack_grid(L2F_STREAM_BYTES), dim3(256), 0, s, w + w2, w + w3, w + wd, base + st.wstream);
                pack_c1();
                break;
            case BT_L2F_WINO:
                pack_c1();
                pack_wino();
                hipLaunchKernelGGL(bt_wino_pack_w3_kernel, pack_grid(WN_W3_BYTES), dim3(256), 0, s, w + wd, base + st.wstream_wino + WN_U_BYTES + WN_W3_BYTES);
                break;
        }
    }
    if (h->uses_zero_page) DF3D_HIP(hipMemsetAsync(base + h->zero_off, 0, 256, s));
    DF3D_LAUNCH_CHECK();
    return DF3D_OK;
}
}  // namespace

// The body of the entry point of the same name (hourglass.hip), whose name the error texts quote through __func__
namespace hg_weights {
int df3d_hg_set_weights(df3d_hg* h, const float* blob_dev, void* lowp_dev, hipStream_t s) {
    DF3D_CHECK_ARG(h && blob_dev, "null argument");
    const float* const blob_caller = blob_dev;
    DF3D_CHECK_ARG((reinterpret_cast<uintptr_t>(blob_dev) & 255) == 0, "blob must be 256-byte aligned");
    if ((h->dtype == DF3D_DTYPE_F16 || h->dtype == DF3D_DTYPE_F32S) && lowp_dev != nullptr) {
        // the half-precision engines need every operand inside the IEEE-half range: refuse weights (biases and folded BatchNorm vectors included)
        // that are not -- here, with the number, instead of as inf / NaN heat-maps later (one 4-byte read-back; the first word of the
        // caller's scratch buffer, which the packers below overwrite, is the reduction's cell)
        unsigned* const cell = reinterpret_cast<unsigned*>(lowp_dev);
        unsigned bits = 0;
        DF3D_HIP(hipMemsetAsync(cell, 0, 4, s));
        hipLaunchKernelGGL(absmax_bits_kernel, dim3(256), dim3(256), 0, s, blob_dev, h->blob_floats, cell);
        DF3D_LAUNCH_CHECK();
        DF3D_HIP(hipMemcpyAsync(&bits, cell, 4, hipMemcpyDeviceToHost, s));
        DF3D_HIP(hipStreamSynchronize(s));
        float absmax;
        memcpy(&absmax, &bits, 4);
        if (!(absmax <= 65504.0f)) {   // (also true for an infinity or a NaN among the weights)
            df3d::set_error("max |w| = %g: the %s hourglass engine needs every weight inside the IEEE-half range (65504): use DF3D_DTYPE_F32 (or BF16)",
                            (double)absmax, h->dtype == DF3D_DTYPE_F16 ? "F16" : "F32S");
            return DF3D_EINVAL;
        }
    }
    if (h->lp()) {
        DF3D_CHECK_ARG(lowp_dev != nullptr, "a 16-bit engine needs a df3d_hg_lowp_bytes() device buffer");
        DF3D_CHECK_ARG((reinterpret_cast<uintptr_t>(lowp_dev) & 255) == 0, "lowp buffer must be 256-byte aligned");
        // the 16-bit copy of the blob; the 16-bit stem wants its weights as a [64][184] tile: overwrite the stem's slot of the copy
        with_elem_type(h->dtype, [&](auto t) {
            using T = decltype(t);
            if constexpr (sizeof(T) == 2) {
                unsigned short* const copy = reinterpret_cast<unsigned short*>(lowp_dev);
                hipLaunchKernelGGL((f32_to_lp_kernel<T>), dim3(1024), dim3(256), 0, s, blob_dev, copy, h->blob_floats);
                hipLaunchKernelGGL((stem_relayout_kernel<T>), dim3(STEM_RELAYOUT_BLOCKS), dim3(256), 0, s, blob_dev + h->steps[0].conv.w_off,
                                   copy + h->steps[0].conv.w_off);
            }
        });
        // (the packers of the 16-bit streams are byte movers: the same kernels serve both formats)
        if (int rc = pack_streams(h, lowp_dev, nullptr, s)) return rc;
        h->lowp = lowp_dev;
    } else if (h->dtype == DF3D_DTYPE_F32S && lowp_dev == nullptr) {
        df3d::set_error("an f32s engine needs a df3d_hg_lowp_bytes() device buffer (the pre-split copy of the weights)");
        return DF3D_EINVAL;
    } else if (h->stream_bytes && lowp_dev == nullptr) {
        // round 1's contract for f32 engines (no scratch buffer): honoured by falling back to the register-staged kernels, which
        // need no weight streams and give bit-identical results.  The parameter manifest does not depend on the option, so the
        // caller's blob stays valid.
        h->ring = 0;
        h->build();
    } else if (h->stream_bytes || h->dtype == DF3D_DTYPE_F32S) {
        DF3D_CHECK_ARG((reinterpret_cast<uintptr_t>(lowp_dev) & 255) == 0, "lowp buffer must be 256-byte aligned");
        if (h->dtype == DF3D_DTYPE_F32S) {
            // f32s: the weights pre-split per 16-float K step (hg_types.h f32s_presplit_kernel) -- a float32-sized copy of the blob in front of
            // the streams; the packers below then read THAT copy (they move whole 16-byte chunks and keep a chunk's index inside its step).
            // Biases and BatchNorm vectors are transformed along with the rest and never read from the copy.
            hipLaunchKernelGGL(f32s_presplit_kernel, dim3(1024), dim3(256), 0, s, reinterpret_cast<const u32x4*>(blob_dev),
                               reinterpret_cast<u32x4*>(lowp_dev), h->blob_floats / 16);
            // the stem's weights: two half-precision [64][184] tiles (hi, lo) in its slot of the copy (exactly the slot's STEM_F32S_W_BYTES)
            hipLaunchKernelGGL(stem_relayout_f32s_kernel, dim3(STEM_RELAYOUT_BLOCKS), dim3(256), 0, s, blob_dev + h->steps[0].conv.w_off,
                               reinterpret_cast<unsigned short*>(reinterpret_cast<float*>(lowp_dev) + h->steps[0].conv.w_off));
            blob_dev = reinterpret_cast<const float*>(lowp_dev);   // (restored below: h->blob stays the caller's float32 blob)
        }
        if (int rc = pack_streams(h, lowp_dev, blob_dev, s)) return rc;
        h->lowp = lowp_dev;
    }
    h->blob = blob_caller;
    return DF3D_OK;
}
}  // namespace hg_weights
