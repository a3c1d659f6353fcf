// a2: stacked-hourglass engine -- layer plan, parameter manifest, workspace planning and launches.
//
// The engine owns WHICH kernel runs on WHICH tensor (the plan below is the 2-stack, depth-4,
// pre-activation-bottleneck hourglass df2d uses: SURVEY.md App. B; constants reference df3d/config.py:18,33,36)
// and nothing else: weights, activations and the stream belong to the caller.
//
// BatchNorm handling (eval mode): a BN that directly follows a convolution (bn2, bn3 inside a bottleneck, the
// stem's bn1, the BN of fc) is folded into that convolution's weights and bias by the HOST packer; the BN on a
// bottleneck's *input* (bn1) cannot be folded because the raw tensor also feeds the skip connection, so it is
// applied as x*scale+shift -> ReLU while the conv1 kernel stages its input tile.
//
// This header is the PLAN, host code only: it takes the kernel headers' layout constants and makes no launch and no HIP runtime call
// (hg_weights.h packs the streams it lays out, hg_launch.h runs its steps; hourglass.hip is the C ABI over the three).
#pragma once
#include <algorithm>
#include <string>
#include <vector>

#include "common.h"
#include "hg_types.h"
#include "hg_conv.h"
#include "hg_stem.h"
#include "hg_pool.h"
#include "hg_bt_reg.h"
#include "hg_bt_ring.h"
#include "hg_bt_l1.h"
#include "hg_head.h"
#include "hg_bt_ring_f32.h"
#include "hg_c1_f32.h"
#include "hg_l1_f32.h"
#include "hg_bt_wino_f32.h"
#include "hg_l1_wino_f32.h"
#include "hg_c1_res_f32.h"

using namespace hgk;

namespace {

enum StepKind { ST_STEM, ST_CONV, ST_POOL, ST_UPADD, ST_BOTTLENECK, ST_HEAD };

// The kernels an ST_BOTTLENECK step runs as, fixed when the plan is built.  The weight streams (Step::wstream*) each form reads, and
// so the ones set_weights packs for it, are listed with it.
enum BtForm {
    BT_REG,         // bottleneck_kernel (hg_bt_reg.h): weights straight from the blob; no streams
    BT_L1_LP,       // 16-bit layer1, bottleneck_l1_kernel (hg_bt_l1.h): wstream = its LDS weight image
    BT_RING_LP,     // 16-bit identity block or layer2, bottleneck_ring_kernel (hg_bt_ring.h): wstream, wstream_w2 (option w2d)
    BT_RING_F32,    // fp32 / f32s identity block, unsplit: bottleneck_ring_f32_kernel (hg_bt_ring_f32.h): wstream
    BT_SPLIT_F32,   // fp32 / f32s identity block: conv1_ring_f32_kernel (hg_c1_f32.h) + the ring tail: wstream_c1, wstream, zero page
    BT_SPLIT_WINO,  // fp32 identity block: conv1_ring_f32_kernel or conv1_res_f32_kernel (option c1res) + bottleneck_wino_f32_kernel:
                    // wstream_c1, wstream_wino (U's first part | W3' | W1 for conv1_res_f32_kernel), wstream_u2, zero page
    BT_L1F,         // fp32 / f32s layer1: conv1_ring_f32_kernel + layer1_tail_f32_kernel (hg_l1_f32.h): wstream_c1, wstream, zero page
    BT_L1F_WINO,    // fp32 layer1: conv1_ring_f32_kernel + layer1_wino_f32_kernel (hg_l1_wino_f32.h): wstream_c1, wstream_wino (U | W3 | Wd),
                    // zero page
    BT_L2F,         // fp32 / f32s layer2: conv1_ring_f32_kernel + layer2_tail_f32_kernel (hg_l1_f32.h): wstream_c1, wstream, zero page
    BT_L2F_WINO,    // fp32 layer2: conv1_ring_f32_kernel + bottleneck_wino_f32_kernel<.., L2>: wstream_c1, wstream_wino (U's first part | W3' |
                    // Wd'), wstream_u2, zero page
};

struct TensorDesc {
    size_t off;  // elements per view, from the start of the activation area
    int h, w, c, pitch;
};

constexpr size_t VIRTUAL_OFF = ~size_t(0);

// BT_L1F_WINO reserves the slot BT_L1F gives its stage images and leaves it unused: nothing packs it, no kernel reads it
constexpr size_t L1F_WINO_UNUSED_SLOT_BYTES = L1F_STREAM_BYTES;

struct ConvPlan {
    int taps, cin, cout, cin_pad, cout_pad;
    bool preact, relu, nchw_out;
    size_t w_off, b_off, s_off, t_off;  // float offsets into the blob (s/t only when preact)
};

struct Step {
    StepKind kind;
    std::string name;
    int in, out, res;  // tensor ids (res = -1: none; UPADD: in = hi-res, res = low-res)
    ConvPlan conv;     // ST_CONV / ST_STEM; for ST_BOTTLENECK: conv = conv1, conv2b = conv2, conv3b = conv3
    ConvPlan conv2b, conv3b, conv4b;  // ST_HEAD: conv = fc, conv2b = score, conv3b = fc_, conv4b = score_
    bool last = false;
    int pool_out = -1;                // ST_BOTTLENECK: tensor receiving the fused 2x2 max-pool of `out`
    int in2 = -1;                     // ST_BOTTLENECK: low-resolution addend of the input (upsample + add fused on the consumer side)
    int add2 = -1;                    // ST_BOTTLENECK: low-resolution addend of the OUTPUT (upsample + add fused into the producer's epilogue)
    BtForm form = BT_REG;             // ST_BOTTLENECK: the kernels it runs as
    int pool_in = -1;                 // ST_BOTTLENECK (ring kernels): tensor receiving the 2x2 max-pool of the block's INPUT
    bool pool_only = false;           // ST_BOTTLENECK (BT_L1_LP, BT_L1F*) whose full-resolution output nobody reads: `out` IS the pooled tensor
    double m1_elems = 0;              // activation elements per view this step moves in the fusion model M1
    int t1 = -1;                      // ST_BOTTLENECK, fp32 split forms (hg_c1_f32.h): the tensor conv1's kernel writes and the tail kernel reads
    // byte offsets of the weight streams behind stream_base() (-1: none)
    long long wstream = -1;           // direct-form stage images (ST_HEAD: Wfc's)
    long long wstream2 = -1;          // ST_HEAD (16-bit, not last): the phase-C stage images
    long long wstream_w2 = -1;        // BT_RING_LP with option w2d: W2' as direct-load MFMA fragments (bt_w2d_pack_kernel)
    long long wstream_c1 = -1;        // fp32 split forms: conv1's stage images
    long long wstream_wino = -1;      // Winograd forms: the Winograd slot (see BtForm)
    long long wstream_u2 = -1;        // BT_SPLIT_WINO, BT_L2F_WINO: U's second part, in the slot the direct form gives its stage images
    int chain = -1;                   // >= 0: planned inside chain number `chain` (frees postponed: its tensors share no memory)
};

struct Allocator {
    // first-fit allocator over "elements per view"; offsets multiple of 64 elements
    struct Blk { size_t off, size; };
    std::vector<Blk> free_list;
    size_t top = 0, peak = 0;
    size_t alloc(size_t n) {
        n = (n + 63) & ~size_t(63);
        for (size_t i = 0; i < free_list.size(); ++i)
            if (free_list[i].size >= n) {
                size_t off = free_list[i].off;
                free_list[i].off += n;
                free_list[i].size -= n;
                if (!free_list[i].size) free_list.erase(free_list.begin() + i);
                return off;
            }
        size_t off = top;
        top += n;
        peak = std::max(peak, top);
        return off;
    }
    void release(size_t off, size_t n) {
        n = (n + 63) & ~size_t(63);
        free_list.push_back({off, n});
        std::sort(free_list.begin(), free_list.end(), [](const Blk& a, const Blk& b) { return a.off < b.off; });
        for (size_t i = 0; i + 1 < free_list.size();) {
            if (free_list[i].off + free_list[i].size == free_list[i + 1].off) {
                free_list[i].size += free_list[i + 1].size;
                free_list.erase(free_list.begin() + i + 1);
            } else
                ++i;
        }
        if (!free_list.empty() && free_list.back().off + free_list.back().size == top) {
            top = free_list.back().off;
            free_list.pop_back();
        }
    }
};

// what the profile records of a launch: flops = the work in the reference's terms, bytes = the least this launch can move (inputs read
// once, outputs written once, intermediates on chip), bytes_m1 = what the fusion model M1 of SURVEY.md 8(d) charges for the same work
// (every convolution's input and output, pooling and upsample passes), flops_executed (< 0: = flops) = what the kernel's MFMAs do
struct Work {
    double flops, bytes, bytes_m1, flops_executed = -1.0;
};

// optional per-kernel-class timing with HIP events on the launch stream (bench.py roofline leg): hg_launch.h records into it
struct HgProfile {
    bool profiling = false;
    struct Timed { hipEvent_t a, b; int cls; Work w; };
    std::vector<std::string> kernel_names;  // class id -> kernel instantiation name (as rocprofv3 prints it, shortened)
    int kernel_class(const std::string& name) {
        for (size_t i = 0; i < kernel_names.size(); ++i)
            if (kernel_names[i] == name) return (int)i;
        kernel_names.push_back(name);
        return (int)kernel_names.size() - 1;
    }
    std::vector<Timed> timed;
    std::vector<hipEvent_t> event_pool;
};

}  // namespace

struct df3d_hg {
    int dtype = DF3D_DTYPE_F32;
    int num_stacks = 2;
    int H = 256, W = 512;
    int classes = 19;
    int rb_override = 0;  // 0 = auto, 64 or 128: staged row bytes per K-step (tuning knob)
    int fuse = 1;         // 1 = 256->128->128->256 bottlenecks at >= 16x32 run as ONE fused kernel
    int fuse_upadd = 1;   // the hourglass' up1 + upsample(low3): 0 = a pass of its own (upadd_kernel); 1 (default) = added in the epilogue of
                          // the bottleneck that produces up1 (the low path runs first) wherever the level's input already has a pooled
                          // copy, consumer side otherwise (measured: +4-5 % frames/s in bf16, +2 % in fp32, bit-identical results); 2 = always folded
                          // into the input load of the consuming bottleneck (round 2)
    int l1 = 1;           // 1 = bf16 layer1 (64 -> 64 -> 64 -> 128) runs as the LDS-resident-weights kernel of hg_bt_l1.h
    int ring = 1;         // 1 = the 256 -> 128 -> 128 -> 256 bottlenecks take their weights through the LDS-DMA ring (hg_bt_ring*.h)
    int w2d = 1;          // 16-bit ring bottlenecks: 1 (default) = the 3x3's weights as direct per-wave fragment loads (hg_bt_ring.h W2D), bit-identical
    int ring2 = 1;        // 16-bit ring bottlenecks (with w2d): 1 (default) = round 4's form (hg_bt_ring.h MODE 2: phase 3 without DMA round trips on its
                          // path, streaming output stores); 0 = round 3's kernels (the A/B); bit-identical either way
    int split1 = 1;       // fp32: 1 (default) = plain 256 -> 128 -> 128 -> 256 blocks run as conv1 (every pixel once) + tail (hg_c1_f32.h), bit-identical
                          // (development: 8 + mask splits only the identity blocks (1), layer1 (2), layer2 (4))
    int wino = 1;         // exact-fp32 engine, split identity blocks: 1 (default) = the tail's 3x3 as Winograd F(2x4, 3x3) (hg_bt_wino_f32.h: 0.455 of the
                          // direct tail's MFMA cycles; fp32 tolerance against the oracle, NOT bit-identical to the direct kernels), 0 = direct implicit GEMM
    int c1res = 1;        // exact-fp32 engine with `wino`: 1 (default) = conv1 of the plain identity blocks with W1 resident in LDS (hg_c1_res_f32.h), bit-identical
                          // to conv1_ring_f32_kernel (0); may be switched between forwards (it changes neither the plan nor the weight streams)
    bool split_id() const { return split1 == 1 || (split1 >= 8 && (split1 & 1)); }
    bool split_l1() const { return split1 == 1 || (split1 >= 8 && (split1 & 2)); }
    bool split_l2() const { return split1 == 1 || (split1 >= 8 && (split1 & 4)); }
    bool uses_zero_page = false;
    size_t zero_off = 0;  // byte offset of 256 zero bytes behind the weight streams (split form: the 3x3 padding of the tail's LDS-DMA)
    int no_reuse = 0;     // 1 = the alias-free workspace plan: no tensor ever takes a released tensor's memory (tests: the default plan must match it bit for bit)
    int chain_views = 0;  // > 0: chains of full-resolution steps run in chunks of this many views (Infinity Cache residency); 0 = off
    std::vector<int> chain_end;   // step i starts a chain [i, chain_end[i]) (chain_end[i] = i + 1: no chain)
    size_t stream_bytes = 0;  // weight streams of all ring bottlenecks (behind the bf16 copy of the blob)
    hgk::StemU8 u8in{nullptr, nullptr, 0, 0, 0, {{0, 0, 0}, {1, 1, 1}, 0}};   // df3d_hg_forward_u8: the stem's input for the duration of that call
    std::vector<TensorDesc> tensors;
    std::vector<int> pooled_of;   // tensor id -> id of its max-pooled copy written by the producing fused bottleneck (-1: none)
    std::vector<Step> steps;
    std::vector<df3d_hg_param> params;
    size_t blob_floats = 0;
    size_t act_elems_per_view = 0;
    const float* blob = nullptr;
    const void* lowp = nullptr;  // bf16 copy of the blob (same offsets, in elements) when dtype = bf16
    double flops_per_view = 0, elems_per_view = 0;

    Allocator alloc;
    HgProfile prof;

    bool lp() const { return dtype == DF3D_DTYPE_BF16 || dtype == DF3D_DTYPE_F16; }   // a 16-bit engine (bf16 or f16: same plan, same kernels, other element type)
    int elem_bytes() const { return lp() ? 2 : 4; }
    // byte offset of the weight streams in the caller's "lowp" buffer: behind the 16-bit copy of the blob (bf16 / f16), at its start (f32)
    // (f32s: behind the pre-split float32 copy of the blob, hg_types.h f32s_presplit_kernel)
    size_t stream_base() const { return lp() ? (blob_floats * 2 + 255) & ~size_t(255) : dtype == DF3D_DTYPE_F32S ? (blob_floats * 4 + 255) & ~size_t(255) : 0; }

    // every step-creating site brackets its accounting: m1_open() before the first elems_per_view update that belongs to the
    // step, push_step(), m1_close() after the last one -> Step::m1_elems
    double m1_mark = 0;
    void m1_open() { m1_mark = elems_per_view; }
    void push_step(const Step& st) {
        steps.push_back(st);
        steps.back().chain = defer_frees ? plan_chain : -1;
    }
    void m1_close() { steps.back().m1_elems = elems_per_view - m1_mark; }
    static Step new_step(StepKind kind, const std::string& name, int in, int res) {
        Step st;
        st.kind = kind;
        st.name = name;
        st.in = in;
        st.res = res;
        return st;
    }
    int new_tensor(int h, int w, int c, int pitch = 0) {
        if (!pitch) pitch = c;
        TensorDesc t{alloc.alloc((size_t)h * w * pitch), h, w, c, pitch};
        tensors.push_back(t);
        pooled_of.push_back(-1);
        return (int)tensors.size() - 1;
    }
    // a tensor that is never materialised (shape only): the full-resolution output of a pooled-output-only bottleneck
    int new_virtual_tensor(int h, int w, int c) {
        tensors.push_back(TensorDesc{VIRTUAL_OFF, h, w, c, c});
        pooled_of.push_back(-1);
        return (int)tensors.size() - 1;
    }
    // While a chain of full-resolution steps is being planned (see chain_end) frees are postponed to its end: the chain runs
    // chunk by chunk, so a tensor released inside it must not lend its memory to a later tensor of the same chain (whose slice
    // for chunk c could overlap the released tensor's slice for chunk c + 1, which is still to be written and read).
    bool defer_frees = false;
    int plan_chain = 0;
    std::vector<int> deferred;
    void free_tensor(int id) {
        if (defer_frees) {
            deferred.push_back(id);
            return;
        }
        const TensorDesc& t = tensors[id];
        if (no_reuse) return;
        if (t.off != VIRTUAL_OFF) alloc.release(t.off, (size_t)t.h * t.w * t.pitch);
    }
    void end_chain() {
        defer_frees = false;
        ++plan_chain;
        for (int id : deferred) free_tensor(id);
        deferred.clear();
    }
    // byte offset of a new weight stream behind stream_base()
    long long take_stream(size_t bytes) {
        const long long off = (long long)stream_bytes;
        stream_bytes += bytes;
        return off;
    }
    size_t add_param(const std::string& name, int kind, int taps, int cin, int cout, int cin_pad, int cout_pad, size_t count,
                     int kperm = 0) {
        df3d_hg_param p;
        memset(&p, 0, sizeof(p));
        p.kperm = kperm;
        snprintf(p.name, sizeof(p.name), "%s", name.c_str());
        p.kind = kind;
        p.taps = taps;
        p.cin = cin;
        p.cout = cout;
        p.cin_pad = cin_pad;
        p.cout_pad = cout_pad;
        p.offset = blob_floats;
        p.count = count;
        blob_floats += (count + 63) & ~size_t(63);
        params.push_back(p);
        return p.offset;
    }

    ConvPlan plan_conv(const std::string& name, int taps, int cin, int cin_pad, int cout, bool preact, bool relu, bool nchw_out,
                       int kperm = 0) {
        const int cout_pad = (cout + 31) / 32 * 32;
        ConvPlan c{taps, cin, cout, cin_pad, cout_pad, preact, relu, nchw_out, 0, 0, 0, 0};
        c.w_off = add_param(name, 0, taps, cin, cout, cin_pad, cout_pad, (size_t)taps * cout_pad * cin_pad, kperm);
        c.b_off = add_param(name, 1, taps, cin, cout, cin_pad, cout_pad, cout_pad);
        if (preact) {
            c.s_off = add_param(name, 2, taps, cin, cout, cin_pad, cout_pad, cin_pad);
            c.t_off = add_param(name, 3, taps, cin, cout, cin_pad, cout_pad, cin_pad);
        }
        return c;
    }
    void account_conv(double px, int taps, int cin, int cout, bool res) {
        flops_per_view += 2.0 * px * taps * cin * cout;
        elems_per_view += px * (cin + cout + (res ? cout : 0));
    }
    // one convolution step; returns the output tensor id
    int conv(const std::string& name, int in, int taps, int cout, bool preact, bool relu, int res, bool nchw_out = false) {
        const TensorDesc ti = tensors[in];
        Step st = new_step(ST_CONV, name, in, res);
        st.conv = plan_conv(name, taps, ti.c, ti.pitch, cout, preact, relu, nchw_out);
        st.out = nchw_out ? -1 : new_tensor(ti.h, ti.w, cout, st.conv.cout_pad);
        m1_open();
        push_step(st);
        account_conv((double)ti.h * ti.w, taps, ti.c, cout, res >= 0);
        m1_close();
        return st.out;
    }
    // x2 >= 0: the block's input is x + nearest-upsample(x2) (the sum an ST_UPADD step would have written into x)
    // only_pool: the caller reads nothing but the max-pooled copy of the output
    // pool_input: the caller also needs max-pool(x) and nobody has produced it: the bf16 ring kernel writes it on the side
    // (pooled_of[x] is set when that happened)
    // a2 >= 0 (identity-skip blocks the fused kernels take; see can_add2): the block writes out + nearest-upsample(a2) under the
    // step name `sum_name` (the tensor an ST_UPADD step would have made of `out`)
    bool can_add2(int x) const {
        const TensorDesc& t = tensors[x];
        return fuse && t.c == 256 && t.h % 8 == 0 && t.w % 16 == 0;
    }
    int bottleneck(const std::string& name, int x, int planes, bool want_pool = false, int x2 = -1, bool only_pool = false, bool pool_input = false,
                   int a2 = -1, const std::string& sum_name = std::string()) {
        const int cin = tensors[x].c, cout = 2 * planes;
        const TensorDesc tx = tensors[x];
        const bool shape_ok = (cin == 256 && planes == 128) || (cin == 128 && planes == 128) || (cin == 64 && planes == 64);
        const bool fused_here = fuse && shape_ok && tx.h % 8 == 0 && tx.w % 16 == 0;
        if (x2 >= 0 && !(fused_here && fuse_upadd && cin == 256 && planes == 128)) {
            upadd(name + ".upadd", x, x2);  // no fused consumer: materialise the sum in place
            x2 = -1;
        }
        if (fused_here) {
            // the whole block in one kernel (hg_bt_reg.h: bottleneck_kernel); algorithmic work is accounted
            // exactly as for the separate convolutions (model M1), although far fewer bytes really move
            const bool ds = cin != cout;
            m1_open();
            Step st;
            st.kind = ST_BOTTLENECK;
            st.name = name + ".conv3";
            st.in = x;
            st.in2 = x2;
            st.add2 = a2;
            if (a2 >= 0) st.name = sum_name;
            if (x2 >= 0 || a2 >= 0) elems_per_view += (double)tx.h * tx.w * cin * 2.25;  // model M1 still counts the upsample + add pass
            st.res = ds ? -1 : x;
            st.conv = plan_conv(name + ".conv1", 1, cin, cin, planes, true, true, false);
            st.conv2b = plan_conv(name + ".conv2", 9, planes, planes, planes, false, true, false);
            if (ds) st.conv4b = plan_conv(name + ".downsample.0", 1, cin, cin, cout, false, false, false);
            st.conv3b = plan_conv(name + ".conv3", 1, planes, planes, cout, false, false, false, lp() ? 1 : 0);
            const bool tiles = tx.h % BT_TH == 0 && tx.w % BT_TW == 0;
            const bool f32 = dtype == DF3D_DTYPE_F32;   // the Winograd forms: the exact-fp32 engine only
            if (ring && lp() && cin == 128 && planes == 128 && x2 < 0 && !want_pool)
                st.form = BT_RING_LP;   // layer2: the same ring kernel with 128 input channels and the skip convolution as eight more stages
            else if (ring && cin == 256 && planes == 128)   // weights through the LDS-DMA ring (hg_bt_ring.h, hg_bt_ring_f32.h)
                st.form = lp() ? BT_RING_LP : !split_id() ? BT_RING_F32 : wino && f32 ? BT_SPLIT_WINO : BT_SPLIT_F32;
            else if (ring && split_l1() && !lp() && cin == 64 && planes == 64 && ds && x2 < 0 && a2 < 0 && tiles)
                st.form = wino && f32 && tx.w % L1W_TW == 0 ? BT_L1F_WINO : BT_L1F;   // Winograd: 8 x 32 tiles
            else if (ring && split_l2() && !lp() && cin == 128 && planes == 128 && ds && x2 < 0 && a2 < 0 && !want_pool && tiles)
                st.form = wino && f32 ? BT_L2F_WINO : BT_L2F;
            else if (l1 && lp() && cin == 64 && planes == 64 && tx.h % 16 == 0 && tx.w % 16 == 0)
                st.form = BT_L1_LP;
            // The Winograd forms keep the direct form's layout, so the buffer's size does not depend on `wino`: U's second part takes
            // the slot of the stage images (layer1 has no second part: L1F_WINO_UNUSED_SLOT_BYTES).  hg_weights.h packs every slot taken here.
            switch (st.form) {
                case BT_REG: break;
                case BT_L1_LP: st.wstream = take_stream(L1_W_BYTES); break;
                case BT_RING_LP:
                    st.wstream = take_stream(br_stream_bytes(cin, ds));
                    if (w2d) st.wstream_w2 = take_stream(BR_W2D_BYTES);
                    break;
                case BT_RING_F32: st.wstream = take_stream(BRF_STREAM_BYTES); break;
                case BT_SPLIT_F32:
                    st.wstream = take_stream(BRF_STREAM_BYTES);
                    st.wstream_c1 = take_stream(c1_stream_bytes(cin));
                    break;
                case BT_SPLIT_WINO:
                    st.wstream_u2 = take_stream(BRF_STREAM_BYTES);
                    st.wstream_c1 = take_stream(c1_stream_bytes(cin));
                    st.wstream_wino = take_stream((size_t)WN_STREAM_BYTES + C1R_W_BYTES);
                    break;
                case BT_L1F:
                    st.wstream = take_stream(L1F_STREAM_BYTES);
                    st.wstream_c1 = take_stream(c1_stream_bytes(cin));
                    break;
                case BT_L1F_WINO:
                    take_stream(L1F_WINO_UNUSED_SLOT_BYTES);
                    st.wstream_c1 = take_stream(c1_stream_bytes(cin));
                    st.wstream_wino = take_stream(L1W_STREAM_BYTES);
                    break;
                case BT_L2F:
                    st.wstream = take_stream(L2F_STREAM_BYTES);
                    st.wstream_c1 = take_stream(c1_stream_bytes(cin));
                    break;
                case BT_L2F_WINO:
                    st.wstream_u2 = take_stream(L2F_STREAM_BYTES);
                    st.wstream_c1 = take_stream(c1_stream_bytes(cin));
                    st.wstream_wino = take_stream(WN_STREAM_BYTES_L2);
                    break;
            }
            if (st.form != BT_REG && cin == 256 && pool_input && x2 < 0 && pooled_of[x] < 0) {   // the ring kernels pool their input on the side
                st.pool_in = new_tensor(tx.h / 2, tx.w / 2, cin);
                pooled_of[x] = st.pool_in;
                elems_per_view += (double)tx.h * tx.w * cin * 1.25;  // model M1 still counts the pooling pass
            }
            if (st.wstream_c1 >= 0) st.t1 = new_tensor(tx.h, tx.w, planes);   // split forms: conv1 on every pixel once, the rest on tiles
            // layer1 (16-bit; fp32 since round 5): the tail writes the pooled tensor only when the full-resolution output (15 of the
            // block's 37 GB per 896 views) has no other reader
            st.pool_only = want_pool && only_pool && (st.form == BT_L1_LP || st.form == BT_L1F || st.form == BT_L1F_WINO);
            int result;
            if (st.pool_only) {
                st.out = new_tensor(tx.h / 2, tx.w / 2, cout);
                result = new_virtual_tensor(tx.h, tx.w, cout);
                pooled_of[result] = st.out;
            } else {
                st.out = result = new_tensor(tx.h, tx.w, cout);
                if (want_pool) {  // the consumer max-pools this tensor: the epilogue writes the pooled copy too (no pool step)
                    st.pool_out = new_tensor(tx.h / 2, tx.w / 2, cout);
                    pooled_of[st.out] = st.pool_out;
                }
            }
            if (want_pool) elems_per_view += (double)tx.h * tx.w * cout * 1.25;  // model M1 still counts the pooling pass
            push_step(st);
            const double px = (double)tx.h * tx.w;
            account_conv(px, 1, cin, planes, false);
            account_conv(px, 9, planes, planes, false);
            if (ds) account_conv(px, 1, cin, cout, false);
            account_conv(px, 1, planes, cout, true);
            m1_close();
            if (st.t1 >= 0) free_tensor(st.t1);
            return result;
        }
        int a = conv(name + ".conv1", x, 1, planes, true, true, -1);
        int b = conv(name + ".conv2", a, 9, planes, false, true, -1);
        free_tensor(a);
        int skip = x;
        if (cin != cout) skip = conv(name + ".downsample.0", x, 1, cout, false, false, -1);
        int o = conv(name + ".conv3", b, 1, cout, false, false, skip);
        free_tensor(b);
        if (skip != x) free_tensor(skip);
        return o;
    }
    int pool(const std::string& name, int x) {
        if (pooled_of[x] >= 0) return pooled_of[x];  // already produced by the fused bottleneck that wrote x
        const TensorDesc t = tensors[x];
        Step st = new_step(ST_POOL, name, x, -1);
        st.out = new_tensor(t.h / 2, t.w / 2, t.c, t.pitch);
        m1_open();
        push_step(st);
        elems_per_view += (double)t.h * t.w * t.c * 1.25;
        m1_close();
        return st.out;
    }
    // hi += upsample(lo), in place on hi
    int upadd(const std::string& name, int hi, int lo) {
        const TensorDesc t = tensors[hi];
        Step st = new_step(ST_UPADD, name, hi, lo);
        st.out = hi;
        m1_open();
        push_step(st);
        elems_per_view += (double)t.h * t.w * t.c * 2.25;
        m1_close();
        return hi;
    }
    // Returns the up-path tensor; *lazy_lo receives the low-path tensor whose upsampled copy still has to be added to it
    // (the consumer -- always a bottleneck -- adds it while loading its input), or -1 when the sum was materialised.
    int hourglass(const std::string& name, int n, int x, int planes, int* lazy_lo) {
        const std::string lv = name + "." + std::to_string(n - 1);
        // LOW PATH FIRST where it can be, then up1 = bottleneck(x) whose epilogue adds upsample(low3) and writes the level's sum: the consumer
        // is a plain block (no second operand in its input load).  Needs max-pool(x) before up1 runs, i.e. a producer that has already
        // written it (everywhere except the second stack's input, which runs up1 first, as in round 2).
        const bool low_first = fuse && fuse_upadd == 1 && can_add2(x) && pooled_of[x] >= 0;
        int up1 = low_first ? -1 : bottleneck(lv + ".0.0", x, planes, false, -1, false, true);
        int low = pool(lv + ".pool", x);   // (low_first: = pooled_of[x])
        int low1 = bottleneck(lv + ".1.0", low, planes, n > 1);
        free_tensor(low);
        int low2, inner_lo = -1;
        if (n > 1)
            low2 = hourglass(name, n - 1, low1, planes, &inner_lo);
        else
            low2 = bottleneck(lv + ".3.0", low1, planes);
        free_tensor(low1);
        int low3 = bottleneck(lv + ".2.0", low2, planes, false, inner_lo);
        free_tensor(low2);
        if (inner_lo >= 0) free_tensor(inner_lo);
        *lazy_lo = -1;
        if (low_first) {
            if (n == 4) defer_frees = chain_views > 0;   // outermost level: this step, the stack's residual block and its head form a chain
            up1 = bottleneck(lv + ".0.0", x, planes, false, -1, false, false, low3, lv + ".upadd");
        } else if (fuse && fuse_upadd) {
            *lazy_lo = low3;   // (freed by the caller, behind the consumer)
            return up1;
        } else {
            upadd(lv + ".upadd", up1, low3);
        }
        free_tensor(low3);
        return up1;
    }

    void build() {
        tensors.clear();
        pooled_of.clear();
        steps.clear();
        params.clear();
        blob_floats = 0;
        stream_bytes = 0;
        alloc = Allocator();
        flops_per_view = elems_per_view = 0;
        deferred.clear();
        plan_chain = 0;
        // chains (chain_views > 0) postpone the frees inside them: a chain's tensors must not share memory.  Without chunking (the
        // default) every tensor is released where its last consumer has run -- round 3 deferred always and planned 65 MB per view in
        // fp32 where 48 suffice (58 against 43 GB for one 896-view step)
        defer_frees = chain_views > 0;   // stem .. layer3 form a chain
        // stem
        Step st = new_step(ST_STEM, "conv1", -1, -1);
        st.conv = ConvPlan{49, 3, 64, 3, 64, false, true, false, 0, 0, 0, 0};
        st.conv.w_off = add_param("conv1", 0, 49, 3, 64, 3, 64, STEM_LP_TILE_ELEMS);  // [148][64] f32 used; slot sized for the 16-bit [64][184] tile (hg_stem.h)
        st.conv.b_off = add_param("conv1", 1, 49, 3, 64, 3, 64, 64);
        st.out = new_tensor(H / 2, W / 2, 64);
        m1_open();
        push_step(st);
        flops_per_view += 2.0 * (H / 2) * (W / 2) * 147 * 64;
        elems_per_view += (double)H * W * 3 + (double)(H / 2) * (W / 2) * 64;
        m1_close();
        int x = st.out;
        int l1 = bottleneck("layer1.0", x, 64, true, -1, true);
        free_tensor(x);
        int p1 = pool("maxpool", l1);
        free_tensor(l1);
        int l2 = bottleneck("layer2.0", p1, 128);
        free_tensor(p1);
        x = bottleneck("layer3.0", l2, 128, true);
        free_tensor(l2);
        end_chain();
        for (int s = 0; s < num_stacks; ++s) {
            const std::string S = std::to_string(s);
            int ylo = -1;
            int y = hourglass("hg." + S + ".hg", 4, x, 128, &ylo);
            int r = bottleneck("res." + S + ".0", y, 128, false, ylo);
            free_tensor(y);
            if (ylo >= 0) free_tensor(ylo);
            if (fuse) {
                // fc -> score -> (fc_, score_) + x in one kernel (hg_head.h: head_kernel)
                const bool last = s == num_stacks - 1;
                const int kp = lp() ? 1 : 0;
                const TensorDesc tr = tensors[r];
                Step st;
                st.kind = ST_HEAD;
                st.last = last;
                if (ring) {   // Wfc through the LDS-DMA stage ring (hg_head.h)
                    st.wstream = take_stream(lp() ? HD_FC_STREAM_BYTES : HD_FC_STREAM_BYTES_F32);
                    if (!last && lp()) st.wstream2 = take_stream(HD_FC2_STREAM_BYTES);
                }
                st.name = last ? "score." + S : "score_." + S;
                st.in = r;
                st.res = last ? -1 : x;
                st.conv = plan_conv("fc." + S + ".0", 1, 256, 256, 256, false, true, false);
                st.conv2b = plan_conv("score." + S, 1, 256, 256, classes, false, false, last, kp);
                const double px = (double)tr.h * tr.w;
                m1_open();
                account_conv(px, 1, 256, 256, false);
                account_conv(px, 1, 256, classes, false);
                if (!last) {
                    st.conv3b = plan_conv("fc_." + S, 1, 256, 256, 256, false, false, false, kp);
                    st.conv4b = plan_conv("score_." + S, 1, classes, 32, 256, false, false, false, kp);
                    account_conv(px, 1, 256, 256, true);
                    account_conv(px, 1, classes, 256, true);
                    st.out = new_tensor(tr.h, tr.w, 256);
                } else {
                    st.out = -1;
                }
                push_step(st);
                m1_close();
                free_tensor(r);
                free_tensor(x);
                end_chain();
                x = st.out;
                continue;
            }
            int f = conv("fc." + S + ".0", r, 1, 256, false, true, -1);
            free_tensor(r);
            const bool last = s == num_stacks - 1;
            int sc = conv("score." + S, f, 1, classes, false, false, -1, last);
            if (!last) {
                int t = conv("fc_." + S, f, 1, 256, false, false, x);
                free_tensor(f);
                free_tensor(x);
                int xn = conv("score_." + S, sc, 1, 256, false, false, t);
                free_tensor(sc);
                free_tensor(t);
                x = xn;
            } else {
                free_tensor(f);
                free_tensor(x);
            }
            end_chain();
        }
        act_elems_per_view = alloc.peak;
        zero_off = stream_bytes;
        uses_zero_page = false;
        for (const Step& st : steps) uses_zero_page = uses_zero_page || st.t1 >= 0;
        if (uses_zero_page) stream_bytes += 256;
        // chains: maximal runs of consecutive steps, each of which reads only the previous step's output (and tensors written
        // before the chain began) at the network's top resolutions
        chain_end.assign(steps.size(), 0);
        for (size_t i = 0; i < steps.size(); ++i) chain_end[i] = (int)i + 1;
        auto big = [&](const Step& st) {
            if (st.kind != ST_STEM && st.kind != ST_BOTTLENECK && st.kind != ST_HEAD) return false;
            const int ref = st.kind == ST_STEM ? st.out : st.in;
            return tensors[ref].h * 4 >= H / 4 * 4 && tensors[ref].h >= H / 4;   // 64 x 128 and above for the 256 x 512 input
        };
        for (size_t i = 0; i < steps.size();) {
            size_t j = i;
            if (big(steps[i])) {
                j = i + 1;
                while (j < steps.size() && big(steps[j]) && steps[j].in == steps[j - 1].out && steps[j].kind != ST_STEM && steps[i].chain >= 0 &&
                       steps[j].chain == steps[i].chain)
                    ++j;
                chain_end[i] = (int)j;
            }
            i = std::max(j, i + 1);
        }
    }
};
