// Replay of scipy.optimize.linear_sum_assignment (SciPy's rectangular shortest-augmenting-path
// solver) by one block: the same assignment as SciPy for every input, ties included.
//
// StrongSORT's min_cost_matching (strongsort/sort/linear_assignment.py:59-78) clamps every cost
// above max_distance to one value, so its matrices are full of equal entries, and which clamped
// column a hopeless row receives decides the order of the unmatched detections, hence the ids of
// the tracks born from them.  An optimal solver with another tie-breaking gives other ids, so the
// solver is replayed step for step rather than replaced:
//   * rows > columns: the transposed problem is solved (and the pairs read back by row);
//   * for each row in order one shortest-augmenting-path search; `remaining` starts as the
//     columns nc-1 ... 0;
//   * a step relaxes every remaining column j from the current row i in float64,
//     r = ((minVal + c[i][j]) - u[i]) - v[j], replacing shortest[j] on r < shortest[j];
//   * it then selects over `remaining` in array order by "strictly lower, or equal and the
//     column is unassigned": the LAST unassigned column among the minima if there is one, else
//     the FIRST minimum.  In parallel this is a minimum over the key (value, rank) with
//     rank = nc - 1 - position for an unassigned column and nc + position for an assigned one;
//   * the selected column leaves `remaining` by moving the last entry into its slot;
//   * u[i] += minVal - shortest[col4row[i]] over the scanned rows (u[cur] += minVal),
//     v[j] -= minVal - shortest[j] over the scanned columns, then the path is flipped.
// The relaxations of a step are independent, the float64 operations are SciPy's in SciPy's
// order (the build has -ffp-contract=off), so the duals and every comparison are bit-identical.
#pragma once
#include "common.hpp"

namespace yta {

constexpr int LSA_T = 512;          // block size of the kernels that call lsa_replay_block
constexpr int LSA_MAX_N = 3072;     // rows / columns whose work arrays fit the 160 KB of LDS

struct LsaWs {
    double *u, *v, *sp;
    int *path, *col4row, *row4col, *remaining, *SR, *SC;
};
__host__ __device__ inline size_t lsa_ws_bytes(int n) { return (size_t)n * (3 * 8 + 6 * 4) + 64; }
__device__ inline LsaWs lsa_ws_carve(unsigned char *p, int n) {
    LsaWs w;
    w.u = (double *)p;
    w.v = w.u + n;
    w.sp = w.v + n;
    w.path = (int *)(w.sp + n);
    w.col4row = w.path + n;
    w.row4col = w.col4row + n;
    w.remaining = w.row4col + n;
    w.SR = w.remaining + n;
    w.SC = w.SR + n;
    return w;
}

struct LsaShared {
    double wval[LSA_T / WAVE];
    int wrank[LSA_T / WAVE];
    int j, r4;
};

// cost: nr0 x nc0, element (i, j) at cost[i * rs + j * cs].  rx[i] (i < nr0) = column of row i or
// -1.  Work arrays in LDS.
// Returns false (block-uniform) when no finite augmenting step exists (a non-finite cost).
__device__ inline bool lsa_replay_block(const double *cost, int nr0, int nc0, long long rs,
                                        long long cs, const LsaWs &w, LsaShared &sh, int *rx) {
    const int t = threadIdx.x, nt = blockDim.x, lane = lane_id(), wid = t / WAVE, nw = nt / WAVE;
    const bool tr = nc0 < nr0;
    const int nr = tr ? nc0 : nr0, nc = tr ? nr0 : nc0;
    const long long si = tr ? cs : rs, sj = tr ? rs : cs;
    for (int i = t; i < nr; i += nt) {
        w.u[i] = 0.0;
        w.col4row[i] = -1;
    }
    for (int j = t; j < nc; j += nt) {
        w.v[j] = 0.0;
        w.row4col[j] = -1;
    }
    auto init_row = [&]() {
        for (int i = t; i < nr; i += nt) w.SR[i] = 0;
        for (int j = t; j < nc; j += nt) {
            w.remaining[j] = nc - 1 - j;
            w.SC[j] = 0;
            w.sp[j] = INFINITY;
        }
    };
    bool ok = true;
    init_row();
    for (int cur = 0; cur < nr && ok; ++cur) {
        block_sync();   // the row's arrays are initialised, the previous path is flipped
        double min_val = 0.0;
        int i = cur, num = nc, sink = -1;
        while (sink == -1) {
            if (t == 0) w.SR[i] = 1;
            const double ui = w.u[i];
            const double *ci = cost + i * si;
            double bv = INFINITY;
            int br = 0x7fffffff;
            for (int it = t; it < num; it += nt) {
                const int j = w.remaining[it];
                const double r = ((min_val + ci[j * sj]) - ui) - w.v[j];
                double s = w.sp[j];
                if (r < s) {
                    w.path[j] = i;
                    w.sp[j] = r;
                    s = r;
                }
                const int rank = w.row4col[j] == -1 ? nc - 1 - it : nc + it;
                if (s < bv || (s == bv && rank < br)) {
                    bv = s;
                    br = rank;
                }
            }
#pragma unroll
            for (int off = 32; off; off >>= 1) {
                const double ov = __shfl_xor(bv, off);
                const int orr = __shfl_xor(br, off);
                if (ov < bv || (ov == bv && orr < br)) {
                    bv = ov;
                    br = orr;
                }
            }
            if (lane == 0) {
                sh.wval[wid] = bv;
                sh.wrank[wid] = br;
            }
            block_sync();
            bv = sh.wval[0];
            br = sh.wrank[0];
            for (int k = 1; k < nw; ++k) {
                const double ov = sh.wval[k];
                const int orr = sh.wrank[k];
                if (ov < bv || (ov == bv && orr < br)) {
                    bv = ov;
                    br = orr;
                }
            }
            if (br == 0x7fffffff || !(bv < INFINITY)) {   // block-uniform
                ok = false;
                break;
            }
            min_val = bv;
            const int it = br < nc ? nc - 1 - br : br - nc;
            if (t == 0) {
                const int j = w.remaining[it];
                sh.j = j;
                sh.r4 = w.row4col[j];
                w.SC[j] = 1;
                w.remaining[it] = w.remaining[num - 1];
            }
            block_sync();
            --num;
            if (sh.r4 == -1) sink = sh.j;
            else i = sh.r4;
        }
        if (!ok) break;
        for (int r = t; r < nr; r += nt)
            if (w.SR[r]) w.u[r] = r == cur ? w.u[r] + min_val : w.u[r] + (min_val - w.sp[w.col4row[r]]);
        for (int j = t; j < nc; j += nt)
            if (w.SC[j]) w.v[j] = w.v[j] - (min_val - w.sp[j]);
        block_sync();   // the dual update reads col4row, SR, SC and sp before they change
        if (t == 0) {
            int j = sink;
            while (true) {
                const int r = w.path[j];
                w.row4col[j] = r;
                const int pj = w.col4row[r];
                w.col4row[r] = j;
                j = pj;
                if (r == cur) break;
            }
        }
        init_row();     // beside the flip: it touches none of path / row4col / col4row
    }
    block_sync();
    if (ok)
        for (int r = t; r < nr0; r += nt) rx[r] = tr ? w.row4col[r] : w.col4row[r];
    block_sync();
    return ok;
}

}  // namespace yta
