// a21 heat-map triangulation (the model is this project's own specification, stated in float64 numpy by
// tests/heatmap3d_oracle.py, whose header lists every operation): the 3-D point of a (frame, joint) is where the sum over the joint's
// views of the logarithm of the view's heat-map, sampled at the point's projection, is largest -- a coarse-to-fine search over 8 x 8 x 8
// points around the start point.  float64, built with -ffp-contract=off, no atomics: two runs give the same bits.
//
// search_kernel: one workgroup of 256 lanes per (frame, joint).
//   window   64 lanes project the 8 corners of the cube the search can reach (5 / 4 of the level-0 cube: a best point on a face moves
//            the next cube past it, by at most 7 / 6 of the half width over all levels) into the 8 views and take, per view, the bounding
//            box of the cells, widened by the four taps and clamped to the plane.  A view that lies behind its camera at all 8 corners
//            says nothing anywhere in the cube and has no window; one that does at some, or a corner that is not finite, makes the
//            window the whole plane.
//   stage    when the windows of the joint's views hold at most `budget` cells together (at most WINDOW_DOUBLES, the LDS array), the
//            logarithm of every cell of every window is taken once and kept in LDS as float64; else nothing is staged.
//   levels   each lane scores two of the level's 512 points; a tap inside its view's window is one LDS read, any other tap (every
//            tap when nothing was staged) reads the plane and takes the logarithm there: the same value, so both routes give the
//            same bits.  The workgroup's arg-max runs under the total order (score descending, index ascending).
// scores_kernel: the score of given points, one lane each, through the same device functions (nothing staged), for the tests.
// counts_kernel: counts [J, 4] from status [n, J], one lane per entry, serial in the frames.
#include <cmath>
#include <cstdint>

#include "buffer_check.h"
#include "geometry_dev.h"

namespace {

using df3d::CamP;
using df3d::MAX_CAM;

constexpr int MAX_J = 64;
constexpr int THREADS = 256;
constexpr int GRID = 8, POINTS = GRID * GRID * GRID;   // config.HEATMAP3D_GRID
constexpr int MAX_LEVELS = 6;
constexpr int WINDOW_DOUBLES = 4096;   // 32 KiB of the CU's 160: four workgroups per CU beside their 6 KiB of other LDS
constexpr int MAX_N = 1 << 20, MAX_M = 1 << 20, MAX_C = 1 << 10, MAX_HW = 1 << 10;
constexpr double REACH = 1.25;

struct Planes {
    short p[MAX_CAM][MAX_J];   // the plane of joint j in view v, or -1
};

struct Window {
    int r0, r1, c0, c1, off;   // cells [r0, r1] x [c0, c1] of the view's plane live at L[off ...], row-major; r1 < r0: nothing staged
};

struct Geometry {
    int V, C, H, W, J;
    unsigned flip;   // bit v: the network saw view v mirrored
    double cell_rows, cell_cols, log_floor;
};

// log(h) where that lies above the floor and h is finite, else the floor: NaN, +-inf, zero and negatives go to the floor
__device__ __forceinline__ double cell_log(float h, double log_floor) {
    const double l = log((double)h);
    return (isfinite(h) && l > log_floor) ? l : log_floor;
}

__device__ __forceinline__ void catmull_rom(double f, double (&w)[4]) {
    w[0] = ((-f + 2.0) * f - 1.0) * f * 0.5;
    w[1] = ((3.0 * f - 5.0) * f * f + 2.0) * 0.5;
    w[2] = ((-3.0 * f + 4.0) * f + 1.0) * f * 0.5;
    w[3] = (f - 1.0) * f * f * 0.5;
}

// (r, c) cells and w of the point under camera Pc; returns whether the view informs: w > 0 and the point inside the plane
__device__ __forceinline__ bool to_cells(const double* Pc, bool flip, const Geometry& g, double x0, double x1, double x2, double& r, double& c) {
    const double u = Pc[0] * x0 + Pc[1] * x1 + Pc[2] * x2 + Pc[3];
    const double v = Pc[4] * x0 + Pc[5] * x1 + Pc[6] * x2 + Pc[7];
    const double w = Pc[8] * x0 + Pc[9] * x1 + Pc[10] * x2 + Pc[11];
    const double col_px = u / w, row_px = v / w;
    r = row_px / g.cell_rows;
    const double cc = col_px / g.cell_cols;
    c = flip ? (double)g.W - cc : cc;
    return w > 0.0 && r >= 0.0 && r <= (double)(g.H - 1) && c >= 0.0 && c <= (double)(g.W - 1);
}

// What one view adds to the score of a point.  plane: the view's [H, W] floats; L: the staged logarithms (win.r1 < win.r0: none)
__device__ __forceinline__ double view_term(const double* Pc, bool flip, const Geometry& g, const float* __restrict__ plane, const double* L,
                                            const Window& win, double x0, double x1, double x2) {
    double r, c;
    if (!to_cells(Pc, flip, g, x0, x1, x2, r, c)) return g.log_floor;
    const double fr = floor(r), fc = floor(c);
    double wr[4], wc[4];
    catmull_rom(r - fr, wr);
    catmull_rom(c - fc, wc);
    const int ir = (int)fr, ic = (int)fc;   // 0 <= r <= H - 1 and 0 <= c <= W - 1 here
    int cols[4];
    bool cols_in = true;
#pragma unroll
    for (int b = 0; b < 4; ++b) {
        const int q = ic - 1 + b;
        cols[b] = q < 0 ? 0 : q > g.W - 1 ? g.W - 1 : q;
        cols_in = cols_in && cols[b] >= win.c0 && cols[b] <= win.c1;
    }
    const int wcols = win.c1 - win.c0 + 1;
    double total = 0.0;
    bool above = false;   // a sample none of whose taps lies above the floor is the floor itself, whatever the weights add up to
#pragma unroll
    for (int a = 0; a < 4; ++a) {
        const int q = ir - 1 + a;
        const int ra = q < 0 ? 0 : q > g.H - 1 ? g.H - 1 : q;
        const bool staged = cols_in && ra >= win.r0 && ra <= win.r1;
        double row = 0.0;
#pragma unroll
        for (int b = 0; b < 4; ++b) {
            const double l = staged ? L[win.off + (ra - win.r0) * wcols + (cols[b] - win.c0)] : cell_log(plane[(size_t)ra * g.W + cols[b]], g.log_floor);
            above = above || l > g.log_floor;
            const double t = wc[b] * l;
            row = b == 0 ? t : row + t;
        }
        const double t = wr[a] * row;
        total = a == 0 ? t : total + t;
    }
    return above && total > g.log_floor ? total : g.log_floor;
}

struct Shared {
    double P[MAX_CAM][12];   // the cameras, read from LDS (a broadcast), as trajectory.hip holds them
    double L[WINDOW_DOUBLES];
    double box[MAX_CAM][8][2];   // the 8 corners' cells per view
    int bad[MAX_CAM][8];
    Window win[MAX_CAM];
    double red_s[THREADS];
    int red_i[THREADS];
};

__global__ __launch_bounds__(THREADS) void search_kernel(CamP cams, Planes planes, Geometry g, const float* __restrict__ hm,
                                                         const double* __restrict__ X0, double half, int levels, int budget,
                                                         double* __restrict__ X, double* __restrict__ score_out, signed char* __restrict__ status,
                                                         int* __restrict__ views_out, double* __restrict__ shift, int* __restrict__ choice,
                                                         signed char* __restrict__ path) {
    __shared__ Shared S;
    const int tid = threadIdx.x;
    const size_t at = blockIdx.x;   // frame * J + joint
    const int frame = (int)(at / g.J), j = (int)(at % g.J);
    const size_t plane_cells = (size_t)g.H * g.W;
    const double x0 = X0[at * 3], x1 = X0[at * 3 + 1], x2 = X0[at * 3 + 2];
    int nviews = 0, mask = 0;
    for (int v = 0; v < g.V; ++v)
        if (planes.p[v][j] >= 0) ++nviews, mask |= 1 << v;
    const bool search = nviews >= 2 && isfinite(x0) && isfinite(x1) && isfinite(x2) && !(x0 == 0.0 && x1 == 0.0 && x2 == 0.0);
    if (!search) {   // the same decision on every lane
        if (tid == 0) {
            X[at * 3] = x0, X[at * 3 + 1] = x1, X[at * 3 + 2] = x2;
            score_out[at] = __builtin_nan("");
            status[at] = 0, views_out[at] = mask, shift[at] = 0.0;
            if (path) path[at] = 0;
        }
        if (tid < levels) choice[at * levels + tid] = -1;
        return;
    }
    if (tid < MAX_CAM * 12) S.P[tid / 12][tid % 12] = cams.p[tid / 12][tid % 12];
    __syncthreads();

    // ---- window: lane (v, k) projects corner k of the reachable cube into view v
    if (tid < MAX_CAM * 8) {
        const int v = tid / 8, k = tid % 8;
        const double e = half * REACH;
        double r = 0.0, c = 0.0;
        int bad = 0;   // 1: the corner lies behind the camera, 2: its cells are not finite
        if (v < g.V && planes.p[v][j] >= 0) {
            const double cx = x0 + ((k & 4) ? e : -e), cy = x1 + ((k & 2) ? e : -e), cz = x2 + ((k & 1) ? e : -e);
            const double* Pc = S.P[v];
            const double w = Pc[8] * cx + Pc[9] * cy + Pc[10] * cz + Pc[11];
            to_cells(Pc, (g.flip >> v) & 1, g, cx, cy, cz, r, c);
            bad = (!isfinite(w) || !isfinite(r) || !isfinite(c)) ? 2 : !(w > 0.0) ? 1 : 0;
        }
        S.box[v][k][0] = r, S.box[v][k][1] = c, S.bad[v][k] = bad;
    }
    __syncthreads();
    if (tid == 0) {
        int used = 0;
        for (int v = 0; v < g.V; ++v) {
            Window w = {0, -1, 0, -1, 0};
            if (planes.p[v][j] >= 0) {
                int behind = 0;
                bool bad = false;
                double rl = S.box[v][0][0], rh = rl, cl = S.box[v][0][1], ch = cl;
                for (int k = 0; k < 8; ++k) {
                    bad = bad || S.bad[v][k] == 2, behind += S.bad[v][k] == 1;
                    rl = fmin(rl, S.box[v][k][0]), rh = fmax(rh, S.box[v][k][0]);
                    cl = fmin(cl, S.box[v][k][1]), ch = fmax(ch, S.box[v][k][1]);
                }
                // w is linear in the point: behind the camera at all 8 corners is behind it in the whole cube, and the view says nothing
                const bool never = !bad && behind == 8;
                bad = bad || (behind > 0 && behind < 8);
                const double Hm = (double)(g.H - 1), Wm = (double)(g.W - 1);
                w.r0 = bad ? 0 : (int)fmin(fmax(floor(rl) - 1.0, 0.0), Hm);
                w.r1 = bad ? g.H - 1 : (int)fmin(fmax(floor(rh) + 2.0, 0.0), Hm);
                w.c0 = bad ? 0 : (int)fmin(fmax(floor(cl) - 1.0, 0.0), Wm);
                w.c1 = bad ? g.W - 1 : (int)fmin(fmax(floor(ch) + 2.0, 0.0), Wm);
                if (never) w.r0 = 0, w.r1 = -1, w.c0 = 0, w.c1 = -1;
                w.off = used;
                used += (w.r1 - w.r0 + 1) * (w.c1 - w.c0 + 1);   // at most MAX_HW^2 a view: no overflow over 8 views
            }
            S.win[v] = w;
        }
        S.red_i[0] = used;
    }
    __syncthreads();
    const bool staged = S.red_i[0] <= budget;   // budget <= WINDOW_DOUBLES: every staged cell has its place in S.L
    __syncthreads();
    if (staged) {
        for (int v = 0; v < g.V; ++v) {
            if (planes.p[v][j] < 0) continue;
            const Window w = S.win[v];
            const int wcols = w.c1 - w.c0 + 1, cells = (w.r1 - w.r0 + 1) * wcols;
            const float* plane = hm + (((size_t)frame * g.V + v) * g.C + planes.p[v][j]) * plane_cells;
            for (int e = tid; e < cells; e += THREADS)
                S.L[w.off + e] = cell_log(plane[(size_t)(w.r0 + e / wcols) * g.W + (w.c0 + e % wcols)], g.log_floor);
        }
    } else if (tid < MAX_CAM) {
        S.win[tid].r0 = 0, S.win[tid].r1 = -1, S.win[tid].c0 = 0, S.win[tid].c1 = -1;
    }
    __syncthreads();

    // ---- the levels
    double base = 0.0;
    for (int v = 0; v < nviews; ++v) base = base + g.log_floor;
    double cx = x0, cy = x1, cz = x2, h = half, best_score = 0.0;
    int st = 1;
    for (int level = 0; level < levels; ++level) {
        const double step = 2.0 * h / (double)GRID;
        double bs = 0.0;
        int bi = 0;
#pragma unroll 1
        for (int q = 0; q < POINTS / THREADS; ++q) {
            const int idx = tid + q * THREADS;
            const double px = cx + ((double)(idx / 64) - 3.5) * step, py = cy + ((double)(idx / 8 % 8) - 3.5) * step,
                         pz = cz + ((double)(idx % 8) - 3.5) * step;
            double s = 0.0;
            for (int v = 0; v < g.V; ++v) {
                if (planes.p[v][j] < 0) continue;
                const float* plane = hm + (((size_t)frame * g.V + v) * g.C + planes.p[v][j]) * plane_cells;
                s = s + view_term(S.P[v], (g.flip >> v) & 1, g, plane, S.L, S.win[v], px, py, pz);
            }
            if (q == 0 || s > bs) bs = s, bi = idx;   // a lane's indices ascend: an equal later score loses
        }
        S.red_s[tid] = bs, S.red_i[tid] = bi;
        __syncthreads();
        for (int o = THREADS / 2; o > 0; o >>= 1) {
            if (tid < o) {
                const double s2 = S.red_s[tid + o];
                const int i2 = S.red_i[tid + o];
                if (s2 > S.red_s[tid] || (s2 == S.red_s[tid] && i2 < S.red_i[tid])) S.red_s[tid] = s2, S.red_i[tid] = i2;
            }
            __syncthreads();
        }
        const double top = S.red_s[0];
        const int best = S.red_i[0];
        __syncthreads();
        best_score = top;
        if (level == 0) {
            if (!(top > base)) {
                st = 2;
                break;
            }
            const int ix = best / 64, iy = best / 8 % 8, iz = best % 8;
            st = (ix == 0 || ix == GRID - 1 || iy == 0 || iy == GRID - 1 || iz == 0 || iz == GRID - 1) ? 3 : 1;
        }
        if (tid == 0) choice[at * levels + level] = best;
        cx = cx + ((double)(best / 64) - 3.5) * step, cy = cy + ((double)(best / 8 % 8) - 3.5) * step, cz = cz + ((double)(best % 8) - 3.5) * step;
        h = step;
    }
    if (st == 2 && tid < levels) choice[at * levels + tid] = -1;
    if (tid == 0) {
        const double ox = st == 2 ? x0 : cx, oy = st == 2 ? x1 : cy, oz = st == 2 ? x2 : cz;
        const double dx = ox - x0, dy = oy - x1, dz = oz - x2;
        X[at * 3] = ox, X[at * 3 + 1] = oy, X[at * 3 + 2] = oz;
        score_out[at] = best_score;
        status[at] = (signed char)st, views_out[at] = mask;
        shift[at] = st == 2 ? 0.0 : sqrt(dx * dx + dy * dy + dz * dz);
        if (path) path[at] = staged ? 1 : 2;
    }
}

__global__ __launch_bounds__(THREADS) void scores_kernel(CamP cams, Planes planes, Geometry g, const float* __restrict__ hm,
                                                         const double* __restrict__ pts, int M, long long total, double* __restrict__ out) {
    __shared__ double P[MAX_CAM][12];
    const int tid = threadIdx.x;
    if (tid < MAX_CAM * 12) P[tid / 12][tid % 12] = cams.p[tid / 12][tid % 12];
    __syncthreads();
    const long long idx = (long long)blockIdx.x * THREADS + tid;
    if (idx >= total) return;
    const long long at = idx / M;
    const int frame = (int)(at / g.J), j = (int)(at % g.J);
    const Window none = {0, -1, 0, -1, 0};
    const double x0 = pts[idx * 3], x1 = pts[idx * 3 + 1], x2 = pts[idx * 3 + 2];
    double s = 0.0;
    for (int v = 0; v < g.V; ++v) {
        if (planes.p[v][j] < 0) continue;
        const float* plane = hm + (((size_t)frame * g.V + v) * g.C + planes.p[v][j]) * (size_t)g.H * g.W;
        s = s + view_term(P[v], (g.flip >> v) & 1, g, plane, nullptr, none, x0, x1, x2);
    }
    out[idx] = s;
}

__global__ __launch_bounds__(THREADS) void counts_kernel(const signed char* __restrict__ status, int n, int J, long long* __restrict__ counts) {
    const int e = blockIdx.x * THREADS + threadIdx.x;
    if (e >= J * 4) return;
    const int j = e / 4, k = e % 4;
    long long c = 0;
    for (int t = 0; t < n; ++t) c += status[(size_t)t * J + j] == k;
    counts[e] = c;
}

}  // namespace

// the checks the two entries share; the nulls of the host arrays come after the ranges, so that n = 0 with no arrays is accepted
#define DF3D_HEATMAP3D_SHAPE()                                                                                   \
    DF3D_CHECK_ARG(n >= 0 && n <= MAX_N, "n must be in [0, 1048576]");                                           \
    DF3D_CHECK_ARG(V >= 1 && V <= MAX_CAM, "V must be in [1, 8]");                                               \
    DF3D_CHECK_ARG(C >= 1 && C <= MAX_C, "C must be in [1, 1024]");                                             \
    DF3D_CHECK_ARG(H >= 4 && H <= MAX_HW && W >= 4 && W <= MAX_HW, "H and W must be in [4, 1024]");              \
    DF3D_CHECK_ARG(J >= 1 && J <= MAX_J, "J must be in [1, 64]");                                                \
    DF3D_CHECK_ARG(cell_rows > 0.0 && cell_cols > 0.0 && std::isfinite(cell_rows) && std::isfinite(cell_cols),   \
                   "cell_rows and cell_cols must be finite and > 0");                                            \
    DF3D_CHECK_ARG(std::isfinite(log_floor) && log_floor < 0.0, "log_floor must be finite and < 0")

static int heatmap3d_tables(const char* fn, const double* P_host, const unsigned char* flip_host, const int* plane_host, int V, int C, int J,
                            CamP& cams, Planes& planes, unsigned& flip) {
    if (!P_host || !flip_host || !plane_host) {
        df3d::set_error("%s: null pointer: %s", fn, !P_host ? "P_host" : !flip_host ? "flip_host" : "plane_host");
        return DF3D_EINVAL;
    }
    memset(&cams, 0, sizeof(cams));
    memcpy(cams.p, P_host, sizeof(double) * 12 * V);
    memset(&planes, 0xff, sizeof(planes));   // -1
    flip = 0;
    for (int v = 0; v < V; ++v) {
        if (flip_host[v]) flip |= 1u << v;
        for (int j = 0; j < J; ++j) {
            const int p = plane_host[v * J + j];
            if (p < -1 || p >= C) {
                df3d::set_error("%s: plane indices must be in [-1, C)", fn);
                return DF3D_EINVAL;
            }
            planes.p[v][j] = (short)p;
        }
    }
    return DF3D_OK;
}

extern "C" int df3d_heatmap3d_window_doubles(void) { return WINDOW_DOUBLES; }

extern "C" int df3d_heatmap3d_scores(const float* hm_dev, int n, int V, int C, int H, int W, const double* P_host, const unsigned char* flip_host,
                                     const int* plane_host, int J, const double* pts_dev, int M, double cell_rows, double cell_cols,
                                     double log_floor, double* out_dev, void* stream) {
    DF3D_HEATMAP3D_SHAPE();
    DF3D_CHECK_ARG(M >= 0 && M <= MAX_M, "M must be in [0, 1048576]");
    if (n == 0 || M == 0) return DF3D_OK;
    CamP cams;
    Planes planes;
    unsigned flip;
    if (const int rc = heatmap3d_tables(__func__, P_host, flip_host, plane_host, V, C, J, cams, planes, flip)) return rc;
    const long long total = (long long)n * J * M;
    DF3D_BUFFERS({"hm", hm_dev, (long long)n * V * C * H * W * 4, 4}, {"pts", pts_dev, total * 24, 8}, {"out", out_dev, total * 8, 8});
    const Geometry g = {V, C, H, W, J, flip, cell_rows, cell_cols, log_floor};
    hipLaunchKernelGGL(scores_kernel, dim3((unsigned)((total + THREADS - 1) / THREADS)), dim3(THREADS), 0, df3d::as_stream(stream), cams, planes, g,
                       hm_dev, pts_dev, M, total, out_dev);
    DF3D_LAUNCH_CHECK();
    return DF3D_OK;
}

extern "C" int df3d_triangulate_heatmaps(const float* hm_dev, int n, int V, int C, int H, int W, const double* P_host,
                                         const unsigned char* flip_host, const int* plane_host, int J, const double* X0_dev, double half,
                                         int levels, double cell_rows, double cell_cols, double log_floor, int budget, double* X_dev,
                                         double* score_dev, signed char* status_dev, int* views_dev, double* shift_dev, int* choice_dev,
                                         long long* counts_dev, signed char* path_dev, void* stream) {
    DF3D_HEATMAP3D_SHAPE();
    DF3D_CHECK_ARG(levels >= 1 && levels <= MAX_LEVELS, "levels must be in [1, 6]");
    DF3D_CHECK_ARG(std::isfinite(half) && half > 0.0, "half must be finite and > 0");
    DF3D_CHECK_ARG(budget >= 0 && budget <= WINDOW_DOUBLES, "budget must be in [0, df3d_heatmap3d_window_doubles()]");
    if (n == 0) return DF3D_OK;
    CamP cams;
    Planes planes;
    unsigned flip;
    if (const int rc = heatmap3d_tables(__func__, P_host, flip_host, plane_host, V, C, J, cams, planes, flip)) return rc;
    const long long nJ = (long long)n * J;
    df3d::Range ranges[10] = {{"hm", hm_dev, (long long)n * V * C * H * W * 4, 4}, {"X0", X0_dev, nJ * 24, 8}, {"X", X_dev, nJ * 24, 8},
                              {"score", score_dev, nJ * 8, 8}, {"status", status_dev, nJ, 1}, {"views", views_dev, nJ * 4, 4},
                              {"shift", shift_dev, nJ * 8, 8}, {"choice", choice_dev, nJ * levels * 4, 4}, {"counts", counts_dev, (long long)J * 32, 8}};
    int count = 9;
    if (path_dev) ranges[count++] = {"path", path_dev, nJ, 1};
    if (const int rc = df3d::check_buffers(__func__, ranges, count)) return rc;
    const Geometry g = {V, C, H, W, J, flip, cell_rows, cell_cols, log_floor};
    hipStream_t st = df3d::as_stream(stream);
    hipLaunchKernelGGL(search_kernel, dim3((unsigned)nJ), dim3(THREADS), 0, st, cams, planes, g, hm_dev, X0_dev, half, levels, budget, X_dev,
                       score_dev, status_dev, views_dev, shift_dev, choice_dev, path_dev);
    hipLaunchKernelGGL(counts_kernel, dim3((unsigned)((J * 4 + THREADS - 1) / THREADS)), dim3(THREADS), 0, st, status_dev, n, J, counts_dev);
    DF3D_LAUNCH_CHECK();
    return DF3D_OK;
}
