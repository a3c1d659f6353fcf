// Pictorial-structures correction of the 2-D detections, three kernels:
//
//   peaks_kernel      (peaks_dev.h, shared with subpixel.hip) top-K local maxima of every heat-map plane.  One 64-lane wave per plane: the 32 KiB plane is staged
//                     through LDS with 16-byte loads, every lane tests its cells against their 8 neighbours in LDS and
//                     keeps a sorted register top-16, K rounds of a wave-wide (value, index) reduction merge the lanes.
//                     HBM-bound: one more read of the heat-maps.
//   proposals_kernel  one workgroup per (frame, joint), one thread per proposal, float64: the two-view DLT of every pair
//                     of peaks of every pair of seeing cameras (the DLT code of df3d_triangulate, geometry_dev.h) + proposal 0,
//                     df3d_triangulate's own output for the arg-max detections; its reprojection score, then the M best by
//                     rank selection in LDS.
//   solve_kernel      one workgroup per (frame, chain): exact min-sum dynamic programming over the M x M bone tables
//                     from the leaf to the root, the backtrack, and the corrected detections in the 38-joint layout.
//
// The model is this project's own specification; tests/pictorial_oracle.py restates it in float64 numpy.
#include <climits>
#include <cmath>

#include "geometry_dev.h"
#include "peaks_dev.h"

namespace {

using df3d::KMAX;

constexpr int MMAX = 256;   // proposals kept per (frame, joint)
constexpr int NJ = 38;      // joints of the skeleton layout
constexpr int NPRED = 19;   // joints the network predicts
constexpr int NCAM = 7;
constexpr int SOLVE_BLOCK = 256;

// ------------------------------------------------------------------------------------------------ shared set-up
struct Setup {
    df3d::CamP cams;    // P of the physical cameras 0..6, pixels
    int pos[NCAM];      // position of physical camera c in camera_ordering
};

// The cameras that see joint j (the re-layout rule), in increasing physical index: at most three.
__device__ __forceinline__ int seeing_cameras(const Setup& su, int j, int* cam, int* src, bool* left) {
    int ns = 0;
    for (int c = 0; c < NCAM; ++c) {
        bool l;
        const int sj = df3d::relayout_source(su.pos[c], j, &l);
        if (sj >= 0 && ns < 3) {
            cam[ns] = c;
            src[ns] = sj;
            left[ns] = l;
            ++ns;
        }
    }
    return ns;
}

__device__ __forceinline__ int clamp_count(int c, int k) { return c < 0 ? 0 : (c > k ? k : c); }
__device__ __forceinline__ int clamp_kept(int c, int m) { return c < 1 ? 1 : (c > m ? m : c); }

// ------------------------------------------------------------------------------------------------ proposals
struct Costs {
    double img_h, img_w, tau, w_r, w_h;
};

__global__ __launch_bounds__(1024) void proposals_kernel(Setup su, Costs co, const double* __restrict__ x0,
                                                         const int* __restrict__ pcount, const float* __restrict__ ppts,
                                                         const float* __restrict__ pval, int T, int t0, int k, int m,
                                                         int* __restrict__ kcount, int* __restrict__ kindex,
                                                         double* __restrict__ kX, double* __restrict__ kU,
                                                         int* __restrict__ kmatch) {
    __shared__ int s_ns, s_cam[3], s_cnt[3];
    __shared__ double s_row[3][KMAX], s_col[3][KMAX], s_val[3][KMAX];
    __shared__ double s_U[3 * KMAX * KMAX + 1];
    __shared__ unsigned char s_ok[3 * KMAX * KMAX + 1];
    const int j = blockIdx.x, tl = blockIdx.y, t = t0 + tl;
    const int tid = threadIdx.x;
    if (tid == 0) {
        int cam[3], src[3];
        bool left[3];
        const int ns = seeing_cameras(su, j, cam, src, left);
        s_ns = ns;
        for (int a = 0; a < 3; ++a) {
            s_cam[a] = a < ns ? cam[a] : 0;
            s_cnt[a] = a < ns ? clamp_count(pcount[((size_t)cam[a] * T + t) * NPRED + src[a]], k) : 0;
        }
        // peak pixels of the seeing cameras, un-flipped exactly as the re-layout does
        for (int a = 0; a < ns; ++a)
            for (int s = 0; s < s_cnt[a]; ++s) {
                const size_t pl = ((size_t)cam[a] * T + t) * NPRED + src[a];
                const double row = (double)ppts[(pl * k + s) * 2 + 0];
                double col = (double)ppts[(pl * k + s) * 2 + 1];
                if (left[a]) col = 1.0 - col;
                s_row[a][s] = row * co.img_h;
                s_col[a][s] = col * co.img_w;
                s_val[a][s] = (double)pval[pl * k + s];
            }
    }
    __syncthreads();
    const int ns = s_ns;
    const int np = 3 * k * k + 1;
    const int npairs = ns * (ns - 1) / 2;

    // this thread's proposal: 0 = DLT of the arg-max detections, else pair q, peak i of camera a, peak jj of camera b
    bool ok = false;
    double X0 = 0.0, X1 = 0.0, X2 = 0.0, U = 0.0;
    int match = 0;
    const int s = tid;
    if (s < np) {
        if (s == 0) {   // df3d_triangulate's point for the arg-max detections (the caller ran that kernel)
            ok = true;
            const size_t o = ((size_t)t * NJ + j) * 3;
            X0 = x0[o];
            X1 = x0[o + 1];
            X2 = x0[o + 2];
        } else {
            const int q = (s - 1) / (k * k), i = ((s - 1) / k) % k, jj = (s - 1) % k;
            const int a = q == 2 ? 1 : 0, b = q == 0 ? 1 : 2;   // pairs (0, 1), (0, 2), (1, 2) of the seeing cameras
            if (q < npairs && i < s_cnt[a] && jj < s_cnt[b]) {
                ok = true;
                double m4[4][4];
#pragma unroll
                for (int u = 0; u < 4; ++u)
#pragma unroll
                    for (int v = 0; v < 4; ++v) m4[u][v] = 0.0;
                int nviews = 0;
                DF3D_DLT_ADD_VIEW(m4, nviews, su.cams.p[s_cam[a]], s_row[a][i], s_col[a][i]);
                DF3D_DLT_ADD_VIEW(m4, nviews, su.cams.p[s_cam[b]], s_row[b][jj], s_col[b][jj]);
                DF3D_DLT_SOLVE(m4, nviews, X0, X1, X2);
            }
        }
        if (ok) {
            const bool finite = isfinite(X0) && isfinite(X1) && isfinite(X2);
            for (int a = 0; a < ns; ++a) {
                const double* p = su.cams.p[s_cam[a]];
                const double u0 = p[0] * X0 + p[1] * X1 + p[2] * X2 + p[3];
                const double u1 = p[4] * X0 + p[5] * X1 + p[6] * X2 + p[7];
                const double u2 = p[8] * X0 + p[9] * X1 + p[10] * X2 + p[11];
                double d = co.tau, hv = 0.0;
                int best = 0;
                if (finite && u2 > 0.0 && s_cnt[a] > 0) {
                    const double x = u0 / u2, y = u1 / u2;   // x = col_px, y = row_px
                    double d2 = __builtin_inf();
                    for (int sl = 0; sl < s_cnt[a]; ++sl) {
                        const double dx = x - s_col[a][sl], dy = y - s_row[a][sl];
                        const double e = dx * dx + dy * dy;
                        if (e < d2) {
                            d2 = e;
                            best = sl;
                        }
                    }
                    if (d2 < __builtin_inf()) {
                        d = sqrt(d2);
                        hv = s_val[a][best];
                    } else {
                        best = 0;
                    }
                }
                const double dd = d < co.tau ? d : co.tau;
                U += co.w_r * (dd * dd) / (co.tau * co.tau) - co.w_h * hv;
                match |= best << (8 * a);
            }
            if (!(U == U)) U = __builtin_inf();
        }
        s_U[s] = U;
        s_ok[s] = ok ? 1 : 0;
    }
    __syncthreads();
    // rank selection: proposal 0 takes kept slot 0, the others the next M - 1 slots by (U, index)
    const size_t tj = (size_t)tl * NJ + j;
    int slot = -1;
    if (s == 0) {
        slot = 0;
        int nvalid = 0;
        for (int q = 1; q < np; ++q) nvalid += s_ok[q];
        kcount[tj] = 1 + (nvalid < m - 1 ? nvalid : m - 1);
    } else if (s < np && ok) {
        int rank = 0;
        for (int q = 1; q < np; ++q)
            if (s_ok[q] && (s_U[q] < U || (s_U[q] == U && q < s))) ++rank;
        if (rank < m - 1) slot = rank + 1;
    }
    if (slot >= 0) {
        const size_t o = tj * m + slot;
        kindex[o] = s;
        kX[o * 3 + 0] = X0;
        kX[o * 3 + 1] = X1;
        kX[o * 3 + 2] = X2;
        kU[o] = U;
        kmatch[o] = match;
    }
}

// ------------------------------------------------------------------------------------------------ solve
struct Chains {
    int n;
    int start[NJ + 1];   // chain c = joint[start[c] .. start[c + 1]), root first
    int joint[NJ];
    double mu[NJ], sigma[NJ];
};

__global__ __launch_bounds__(SOLVE_BLOCK) void solve_kernel(Setup su, Chains ch, double w_b, const double* __restrict__ am,
                                                            const int* __restrict__ pcount, const float* __restrict__ ppts,
                                                            int T, int t0, int k, int m, const int* __restrict__ kcount,
                                                            const int* __restrict__ kindex, const double* __restrict__ kX,
                                                            const double* __restrict__ kU, const int* __restrict__ kmatch,
                                                            double* __restrict__ out, int* __restrict__ choice,
                                                            double* __restrict__ chain_energy) {
    __shared__ double s_cost[MMAX], s_new[MMAX], s_X[MMAX][3];
    __shared__ unsigned char s_arg[NJ - 1][MMAX];
    __shared__ int s_choice[NJ];
    const int cidx = blockIdx.x, tl = blockIdx.y, t = t0 + tl;
    const int tid = threadIdx.x;
    const int first = ch.start[cidx], L = ch.start[cidx + 1] - first;
    const int* jo = ch.joint + first;
    const size_t row = (size_t)tl * NJ;

    // the leaf's own costs
    int nc = clamp_kept(kcount[row + jo[L - 1]], m);
    for (int x = tid; x < nc; x += SOLVE_BLOCK) {
        const size_t o = (row + jo[L - 1]) * m + x;
        s_cost[x] = kU[o];
        s_X[x][0] = kX[o * 3 + 0];
        s_X[x][1] = kX[o * 3 + 1];
        s_X[x][2] = kX[o * 3 + 2];
    }
    __syncthreads();
    for (int e = L - 1; e >= 1; --e) {   // bone (jo[e - 1], jo[e]): message to the parent
        const int child = jo[e], par = jo[e - 1];
        const int np = clamp_kept(kcount[row + par], m);
        const double mu = ch.mu[child], isg = 1.0 / ch.sigma[child];
        for (int x = tid; x < np; x += SOLVE_BLOCK) {
            const size_t o = (row + par) * m + x;
            const double px = kX[o * 3 + 0], py = kX[o * 3 + 1], pz = kX[o * 3 + 2];
            double best = __builtin_inf();
            int arg = 0;
            for (int y = 0; y < nc; ++y) {
                const double dx = px - s_X[y][0], dy = py - s_X[y][1], dz = pz - s_X[y][2];
                const double z = (sqrt(dx * dx + dy * dy + dz * dz) - mu) * isg;
                const double v = s_cost[y] + w_b * (z * z);
                if (v < best) {
                    best = v;
                    arg = y;
                }
            }
            s_new[x] = kU[o] + best;
            s_arg[e - 1][x] = (unsigned char)arg;
        }
        __syncthreads();
        for (int x = tid; x < np; x += SOLVE_BLOCK) {
            const size_t o = (row + par) * m + x;
            s_cost[x] = s_new[x];
            s_X[x][0] = kX[o * 3 + 0];
            s_X[x][1] = kX[o * 3 + 1];
            s_X[x][2] = kX[o * 3 + 2];
        }
        nc = np;
        __syncthreads();
    }
    if (tid == 0) {   // the root's argmin, then the backtrack to the leaf
        double best = __builtin_inf();
        int arg = 0;
        for (int x = 0; x < nc; ++x)
            if (s_cost[x] < best) {
                best = s_cost[x];
                arg = x;
            }
        s_choice[0] = arg;
        for (int e = 1; e < L; ++e) s_choice[e] = s_arg[e - 1][s_choice[e - 1]];
        chain_energy[(size_t)tl * ch.n + cidx] = best;
    }
    __syncthreads();
    // outputs: one thread per (joint of the chain, camera)
    for (int w = tid; w < L * NCAM; w += SOLVE_BLOCK) {
        const int e = w / NCAM, c = w % NCAM, j = jo[e];
        const size_t o = (row + j) * m + s_choice[e];
        if (c == 0) choice[(size_t)t * NJ + j] = kindex[o];
        bool left;
        const int src = df3d::relayout_source(su.pos[c], j, &left);
        const size_t oi = (((size_t)c * T + t) * NJ + j) * 2;
        double r = am[oi], cl = am[oi + 1];
        if (src >= 0) {
            int rank = 0;   // this camera's place among the cameras that see j (the byte of the match word)
            for (int c2 = 0; c2 < c; ++c2) {
                bool l2;
                rank += df3d::relayout_source(su.pos[c2], j, &l2) >= 0;
            }
            const size_t pl = ((size_t)c * T + t) * NPRED + src;
            const int cnt = clamp_count(pcount[pl], k);
            if (cnt > 0) {
                const int sl = min((kmatch[o] >> (8 * rank)) & 0xff, cnt - 1);
                r = (double)ppts[(pl * k + sl) * 2 + 0];
                cl = (double)ppts[(pl * k + sl) * 2 + 1];
                if (left) cl = 1.0 - cl;
            }
        }
        out[oi] = r;
        out[oi + 1] = cl;
    }
}

__global__ void energy_kernel(const double* __restrict__ chain_energy, int nchains, int t0, int tn, double* __restrict__ energy) {
    const int tl = blockIdx.x * blockDim.x + threadIdx.x;
    if (tl >= tn) return;
    double e = 0.0;
    for (int c = 0; c < nchains; ++c) e += chain_energy[(size_t)tl * nchains + c];
    energy[t0 + tl] = e;
}

int setup_from_host(const double* P_host, const int* ordering_host, Setup* su) {
    memset(su, 0, sizeof(*su));
    int seen = 0;
    for (int k = 0; k < NCAM; ++k) {
        DF3D_CHECK_ARG(ordering_host[k] >= 0 && ordering_host[k] < NCAM, "camera ordering entries must be in [0, 6]");
        seen |= 1 << ordering_host[k];
        su->pos[ordering_host[k]] = k;
    }
    DF3D_CHECK_ARG(seen == 0x7f, "camera ordering must be a permutation of 0..6");
    for (int i = 0; i < NCAM * 12; ++i) DF3D_CHECK_ARG(std::isfinite(P_host[i]), "projection matrices must be finite");
    memcpy(su->cams.p, P_host, sizeof(double) * 12 * NCAM);
    return DF3D_OK;
}

int check_frames(int T, int t0, int tn, int k, int m) {
    DF3D_CHECK_ARG(T >= 0 && t0 >= 0 && tn >= 0 && (long long)t0 + tn <= T, "frame range [t0, t0 + tn) must lie in [0, T)");
    DF3D_CHECK_ARG(k >= 1 && k <= KMAX, "k must be in [1, 16]");
    DF3D_CHECK_ARG(m >= 1 && m <= MMAX, "m must be in [1, 256]");
    DF3D_CHECK_ARG(tn <= 65535, "at most 65535 frames per call");
    return DF3D_OK;
}

}  // namespace

extern "C" int df3d_heatmap_peaks(const float* hm_dev, int n, int joints, int h, int w, int k, int* count_dev, float* pts_dev,
                                  float* val_dev, void* stream) {
    DF3D_CHECK_ARG(n >= 0 && joints > 0 && h > 0 && w > 0, "bad shape");
    DF3D_CHECK_ARG(k >= 1 && k <= KMAX, "k must be in [1, 16]");
    DF3D_CHECK_ARG(((h & (h - 1)) == 0) && ((w & (w - 1)) == 0), "h and w must be powers of two (reference heat-maps are 64 x 128)");
    DF3D_CHECK_ARG(h * w >= 64 && h * w <= 8192, "a plane must hold 64 .. 8192 cells (it is staged in LDS, 128 cells per lane)");
    if (n == 0) return DF3D_OK;
    DF3D_CHECK_ARG(hm_dev && count_dev && pts_dev && val_dev, "null pointer");
    DF3D_CHECK_ARG((reinterpret_cast<uintptr_t>(hm_dev) & 15) == 0, "heat-maps must be 16-byte aligned");
    const long long planes = (long long)n * joints;
    DF3D_CHECK_ARG(planes < (1ll << 31), "too many planes");
    const int wshift = __builtin_ctz((unsigned)w);
    hipLaunchKernelGGL(df3d::peaks_kernel<false>, dim3((unsigned)planes), dim3(df3d::PEAK_BLOCK), sizeof(float) * h * w, df3d::as_stream(stream),
                       hm_dev, h * w, w, wshift, k, 1.0f / (float)h, 1.0f / (float)w, count_dev, pts_dev, val_dev);
    DF3D_LAUNCH_CHECK();
    return DF3D_OK;
}

extern "C" int df3d_ps_proposals(const double* P_host, const int* ordering_host, const double* X0_dev,
                                 const int* peak_count_dev, const float* peak_pts_dev, const float* peak_val_dev, int T, int t0,
                                 int tn, int k, int m, double img_h, double img_w, double tau, double w_reproj, double w_heatmap,
                                 int* kept_count_dev, int* kept_index_dev, double* kept_X_dev, double* kept_U_dev,
                                 int* kept_match_dev, void* stream) {
    if (int rc = check_frames(T, t0, tn, k, m)) return rc;
    DF3D_CHECK_ARG(img_h > 0 && img_w > 0 && std::isfinite(img_h) && std::isfinite(img_w), "image shape must be positive");
    DF3D_CHECK_ARG(tau > 0 && std::isfinite(tau), "tau must be positive");
    DF3D_CHECK_ARG(std::isfinite(w_reproj) && std::isfinite(w_heatmap), "weights must be finite");
    DF3D_CHECK_ARG(P_host && ordering_host, "null pointer");
    Setup su;
    if (int rc = setup_from_host(P_host, ordering_host, &su)) return rc;
    if (tn == 0) return DF3D_OK;
    DF3D_CHECK_ARG(X0_dev && peak_count_dev && peak_pts_dev && peak_val_dev && kept_count_dev && kept_index_dev && kept_X_dev &&
                       kept_U_dev && kept_match_dev, "null pointer");
    const int np = 3 * k * k + 1;
    const int threads = (np + 63) / 64 * 64;
    Costs co{img_h, img_w, tau, w_reproj, w_heatmap};
    hipLaunchKernelGGL(proposals_kernel, dim3(NJ, tn), dim3(threads), 0, df3d::as_stream(stream), su, co, X0_dev,
                       peak_count_dev, peak_pts_dev, peak_val_dev, T, t0, k, m, kept_count_dev, kept_index_dev, kept_X_dev,
                       kept_U_dev, kept_match_dev);
    DF3D_LAUNCH_CHECK();
    return DF3D_OK;
}

extern "C" int df3d_ps_solve(const int* ordering_host, const int* parent_host, const double* bone_host, double w_bone,
                             const double* argmax2d_dev, const int* peak_count_dev, const float* peak_pts_dev, int T, int t0,
                             int tn, int k, int m, const int* kept_count_dev, const int* kept_index_dev,
                             const double* kept_X_dev, const double* kept_U_dev, const int* kept_match_dev,
                             double* points2d_dev, int* choice_dev, double* energy_dev, double* work_dev,
                             size_t work_doubles, void* stream) {
    if (int rc = check_frames(T, t0, tn, k, m)) return rc;
    DF3D_CHECK_ARG(std::isfinite(w_bone), "w_bone must be finite");
    DF3D_CHECK_ARG(ordering_host && parent_host && bone_host, "null pointer");
    static const double no_projection[NCAM * 12] = {};
    Setup su;
    if (int rc = setup_from_host(no_projection, ordering_host, &su)) return rc;
    // the tree: every joint has at most one parent and one child, so it is a set of chains; listed root first, roots in
    // increasing joint order
    Chains ch;
    memset(&ch, 0, sizeof(ch));
    int child[NJ];
    for (int j = 0; j < NJ; ++j) child[j] = -1;
    for (int j = 0; j < NJ; ++j) {
        const int p = parent_host[j];
        DF3D_CHECK_ARG(p >= -1 && p < NJ && p != j, "parent entries must be -1 or another joint in [0, 37]");
        if (p >= 0) {
            DF3D_CHECK_ARG(child[p] < 0, "a joint may be the parent of one joint only (the tree must be a set of chains)");
            child[p] = j;
            DF3D_CHECK_ARG(std::isfinite(bone_host[2 * j]) && bone_host[2 * j + 1] > 0 && std::isfinite(bone_host[2 * j + 1]),
                           "bone length mean must be finite and its deviation positive");
            ch.mu[j] = bone_host[2 * j];
            ch.sigma[j] = bone_host[2 * j + 1];
        }
    }
    int placed = 0;
    for (int r = 0; r < NJ; ++r) {
        if (parent_host[r] >= 0) continue;
        ch.start[ch.n++] = placed;
        for (int j = r; j >= 0 && placed < NJ; j = child[j]) ch.joint[placed++] = j;
    }
    ch.start[ch.n] = placed;
    DF3D_CHECK_ARG(placed == NJ, "the parent table has a cycle");
    if (tn == 0) return DF3D_OK;
    DF3D_CHECK_ARG(argmax2d_dev && peak_count_dev && peak_pts_dev && kept_count_dev && kept_index_dev && kept_X_dev && kept_U_dev &&
                       kept_match_dev && points2d_dev && choice_dev && energy_dev && work_dev, "null pointer");
    DF3D_CHECK_ARG(work_doubles >= (size_t)NJ * tn, "work buffer too small: 38 doubles per frame");
    hipLaunchKernelGGL(solve_kernel, dim3(ch.n, tn), dim3(SOLVE_BLOCK), 0, df3d::as_stream(stream), su, ch, w_bone, argmax2d_dev,
                       peak_count_dev, peak_pts_dev, T, t0, k, m, kept_count_dev, kept_index_dev, kept_X_dev, kept_U_dev,
                       kept_match_dev, points2d_dev, choice_dev, work_dev);
    DF3D_LAUNCH_CHECK();
    hipLaunchKernelGGL(energy_kernel, dim3((tn + 255) / 256), dim3(256), 0, df3d::as_stream(stream), work_dev, ch.n, t0, tn,
                       energy_dev);
    DF3D_LAUNCH_CHECK();
    return DF3D_OK;
}
