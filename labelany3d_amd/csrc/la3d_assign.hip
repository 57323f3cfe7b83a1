// la3d_assign.hip - the assignment on the device (include/la3d.h "assignment on the device"): for every group - an image - the
// rectangular linear sum assignment of its na x nb matrix, SciPy's shortest-augmenting-path solver step for step, ties included.
//   one wave per group, no barriers: every step of the solver is a wave-wide step over the remaining columns.
//   column j    lives in lane j % 64, slot j / 64 (LA3D_ASSIGN_MAX_N / 64 slots): its path cost sp, its dual v, its row row4col,
//               its predecessor path and its position in SciPy's `remaining` list are registers.
//   rows        the duals u and col4row in LDS; the row set SR needs no table: the rows of SR other than the current one are the
//               rows of the visited columns, so the dual update walks the visited columns.
//   the choice  SciPy scans `remaining` by ascending position and takes a new column when its cost is lower, or equal with no row
//               yet.  In parallel: of the columns with the least cost, an unassigned one at the HIGHEST position, else the one at
//               the LOWEST position - one key per column (unassigned: nc - 1 - position; assigned: nc + position), the least key
//               wins.  A wave minimum of the cost, a wave minimum of the key, a ballot for the winner's lane.
//   the matrix  staged into LDS in the solver's orientation (transposed where na > nb) while it is scanned for NaN / -inf, when it
//               has at most LA3D_ASSIGN_STAGE_MAX elements; a larger one is read where it lies (a row of the solver is then a
//               column of the matrix where na > nb).  The values and their order of use are the same: so are the results.
// Only additions and subtractions of float64 occur: there is nothing for fma contraction to change.
#include <cstdint>
#include <cstddef>
#include <climits>
#include <cmath>

#include "la3d_device.hpp"

using namespace la3d;

namespace {
constexpr int MAX_N = LA3D_ASSIGN_MAX_N;
constexpr int SLOTS = MAX_N / 64;
constexpr int STAGE = LA3D_ASSIGN_STAGE_MAX;
constexpr int GONE = -2;     // position of a column that is in SC (visited); -1: the slot holds no column

struct AssignParams {
  const void* cost; long long ncost;
  const long long* offsets; const int* row_a; const int* row_b;
  long long rows_a, rows_b;
  int* col_of_row; int* row_of_col; int* status;
  int maximize;
};

__device__ inline int uniform_i32(int v) { return __builtin_amdgcn_readfirstlane(v); }
template <bool I32>
__device__ __forceinline__ double cost_at(const void* base, long long at, bool neg) {
  const double c = I32 ? (double)static_cast<const int*>(base)[at] : static_cast<const double*>(base)[at];
  return neg ? -c : c;
}
__device__ __forceinline__ int pick(const int (&x)[SLOTS], int s) {
  int r = x[0];
#pragma unroll
  for (int t = 1; t < SLOTS; ++t) r = s == t ? x[t] : r;
  return r;
}
// every row and column of the group unmatched, and its status
__device__ inline void leave(const AssignParams& p, int g, int a0, int na, int b0, int nb, int lane, int status) {
  for (int k = lane; k < na; k += 64) p.col_of_row[a0 + k] = -1;
  for (int k = lane; k < nb; k += 64) p.row_of_col[b0 + k] = -1;
  if (lane == 0) p.status[g] = status;
}

template <bool I32>
__global__ __launch_bounds__(64) void assign_kernel(const AssignParams p) {
  __shared__ double stage[STAGE];
  __shared__ double u[MAX_N];
  __shared__ int col4row[MAX_N];
  const int g = blockIdx.x, lane = threadIdx.x;
  // the tables (uniform), checked before an address is formed from them
  const int a0 = uniform_i32(p.row_a[g]), a1 = uniform_i32(p.row_a[g + 1]);
  const int b0 = uniform_i32(p.row_b[g]), b1 = uniform_i32(p.row_b[g + 1]);
  const long long off = uniform_i64(p.offsets[g]);
  const long long nal = (long long)a1 - a0, nbl = (long long)b1 - b0;
  if (nal < 0 || nbl < 0 || a0 < 0 || a1 > p.rows_a || b0 < 0 || b1 > p.rows_b || off < 0 || off > p.ncost || nal * nbl > p.ncost - off) {
    if (lane == 0) p.status[g] = LA3D_ASSIGN_BROKEN;
    return;
  }
  const int na = (int)nal, nb = (int)nbl;
  if (na == 0 || nb == 0) return leave(p, g, a0, na, b0, nb, lane, LA3D_ASSIGN_OK);
  if (na > MAX_N || nb > MAX_N) return leave(p, g, a0, na, b0, nb, lane, LA3D_ASSIGN_TOO_LARGE);
  const bool tr = na > nb, neg = p.maximize != 0;
  const int nr = tr ? nb : na, nc = tr ? na : nb;   // the solver's rows and columns: nr <= nc
  const bool staged = nr * nc <= STAGE;
  // one pass over the matrix where it lies (coalesced): the invalid entries, and the LDS image in the solver's orientation
  bool bad = false;
  for (int k = lane; k < na * nb; k += 64) {
    const double c = cost_at<I32>(p.cost, off + k, neg);
    if (!I32) bad = bad || c != c || c == -INFINITY;
    if (staged) {
      const int ia = k / nb, jb = k - ia * nb;
      stage[tr ? jb * nc + ia : k] = c;
    }
  }
  if (__ballot(bad) != 0) return leave(p, g, a0, na, b0, nb, lane, LA3D_ASSIGN_INVALID);
  for (int k = lane; k < nr; k += 64) { u[k] = 0.0; col4row[k] = -1; }
  double v[SLOTS], sp[SLOTS];
  int row4col[SLOTS], path[SLOTS], pos[SLOTS];
#pragma unroll
  for (int s = 0; s < SLOTS; ++s) { v[s] = 0.0; row4col[s] = -1; }
  for (int cur = 0; cur < nr; ++cur) {
#pragma unroll
    for (int s = 0; s < SLOTS; ++s) {
      const int j = lane + 64 * s;
      sp[s] = INFINITY; path[s] = -1; pos[s] = j < nc ? nc - 1 - j : -1;
    }
    int nrem = nc, i = cur, sink = -1;
    double minv = 0.0;
    while (true) {
      const double ui = u[i];
      double c[SLOTS];
#pragma unroll
      for (int s = 0; s < SLOTS; ++s) {
        const int j = lane + 64 * s;
        c[s] = 0.0;
        if (pos[s] >= 0) c[s] = staged ? stage[i * nc + j] : cost_at<I32>(p.cost, off + (tr ? (long long)j * nb + i : (long long)i * nb + j), neg);
      }
      double best = INFINITY;
      int bkey = INT_MAX, bslot = 0, brow = -1;
#pragma unroll
      for (int s = 0; s < SLOTS; ++s) {
        if (pos[s] >= 0) {
          const double r = ((minv + c[s]) - ui) - v[s];
          if (r < sp[s]) { path[s] = i; sp[s] = r; }
          const int key = row4col[s] == -1 ? nc - 1 - pos[s] : nc + pos[s];
          if (sp[s] < best || (sp[s] == best && key < bkey)) { best = sp[s]; bkey = key; bslot = s; brow = row4col[s]; }
        }
      }
      const double lowest = wave_min(best);
      if (lowest == INFINITY) return leave(p, g, a0, na, b0, nb, lane, LA3D_ASSIGN_INFEASIBLE);   // (uniform)
      const int wkey = wave_min_i(best == lowest ? bkey : INT_MAX);
      const int wl = __builtin_ctzll(__ballot(best == lowest && bkey == wkey));   // the one lane that holds the chosen column
      const int ws = __builtin_amdgcn_readlane(bslot, wl), wrow = __builtin_amdgcn_readlane(brow, wl);
      minv = readlane_f64(best, wl);
      // remaining[index] = remaining[--nrem]; the chosen column joins SC
      const int index = wkey < nc ? nc - 1 - wkey : wkey - nc;
      --nrem;
#pragma unroll
      for (int s = 0; s < SLOTS; ++s) {
        if (pos[s] == nrem) pos[s] = index;
        if (lane == wl && s == ws) pos[s] = GONE;
      }
      if (wrow == -1) { sink = wl + 64 * ws; break; }
      i = wrow;
    }
    // the duals: u[cur] += minv; u[i] += minv - sp[col4row[i]] for the other rows of SR, by way of their columns; v[j] -= minv - sp[j]
    if (lane == 0) u[cur] += minv;
#pragma unroll
    for (int s = 0; s < SLOTS; ++s) {
      if (pos[s] == GONE) {
        if (lane + 64 * s != sink) u[row4col[s]] += minv - sp[s];
        v[s] -= minv - sp[s];
      }
    }
    // augment along the path from the sink back to cur
    int j = sink;
    for (int step = 0; step < nr; ++step) {   // (a path has at most nr columns)
      const int s = j >> 6, l = j & 63;
      const int r = __builtin_amdgcn_readlane(pick(path, s), l);
#pragma unroll
      for (int t = 0; t < SLOTS; ++t)
        if (lane == l && t == s) row4col[t] = r;
      const int next = col4row[r];
      if (lane == 0) col4row[r] = j;
      j = next;
      if (r == cur) break;
    }
  }
  // the solver's rows are A's, or B's where the transpose was solved
  for (int k = lane; k < nr; k += 64) {
    if (tr) p.row_of_col[b0 + k] = col4row[k];
    else p.col_of_row[a0 + k] = col4row[k];
  }
#pragma unroll
  for (int s = 0; s < SLOTS; ++s) {
    const int jj = lane + 64 * s;
    if (jj < nc) {
      if (tr) p.col_of_row[a0 + jj] = row4col[s];
      else p.row_of_col[b0 + jj] = row4col[s];
    }
  }
  if (lane == 0) p.status[g] = LA3D_ASSIGN_OK;
}

inline uintptr_t at(const void* q) { return reinterpret_cast<uintptr_t>(q); }
}  // namespace

extern "C" {

int la3d_assign(const la3d_assign_args* args) {
  const char* who = "la3d_assign";
  if (!args || args->struct_size != (int32_t)sizeof(la3d_assign_args)) return refuse(who, "NULL block or a struct_size that is not sizeof(la3d_assign_args)");
  const la3d_assign_args& a = *args;
  if (a.G < 0 || a.rows_a < 0 || a.rows_b < 0 || a.ncost < 0) return refuse(who, "negative G, rows_a, rows_b or ncost");
  if (a.cost_dtype != LA3D_ASSIGN_F64 && a.cost_dtype != LA3D_ASSIGN_I32) return refuse(who, "cost_dtype must be LA3D_ASSIGN_F64 or LA3D_ASSIGN_I32");
  if (a.maximize != 0 && a.maximize != 1) return refuse(who, "maximize must be 0 or 1");
  if (a.G == 0) return LA3D_SUCCESS;
  if (!a.offsets || !a.row_offsets_a || !a.row_offsets_b || !a.status || (a.ncost > 0 && !a.cost) || (a.rows_a > 0 && !a.col_of_row) ||
      (a.rows_b > 0 && !a.row_of_col))
    return refuse(who, "NULL cost, offsets, row_offsets_a, row_offsets_b, col_of_row, row_of_col or status");
  if ((at(a.cost) & (a.cost_dtype == LA3D_ASSIGN_F64 ? 7 : 3)) || (at(a.offsets) & 7))
    return refuse(who, "cost not aligned to its element, or offsets not an 8-byte aligned pointer");
  if ((at(a.row_offsets_a) | at(a.row_offsets_b) | at(a.col_of_row) | at(a.row_of_col) | at(a.status)) & 3)
    return refuse(who, "row_offsets_a, row_offsets_b, col_of_row, row_of_col or status not a 4-byte aligned pointer");
  const AssignParams p = {a.cost, a.ncost, reinterpret_cast<const long long*>(a.offsets), a.row_offsets_a, a.row_offsets_b, a.rows_a, a.rows_b,
                          a.col_of_row, a.row_of_col, a.status, a.maximize};
  hipStream_t st = static_cast<hipStream_t>(a.stream);
  if (a.cost_dtype == LA3D_ASSIGN_I32) hipLaunchKernelGGL(assign_kernel<true>, dim3((unsigned)a.G), dim3(64), 0, st, p);
  else hipLaunchKernelGGL(assign_kernel<false>, dim3((unsigned)a.G), dim3(64), 0, st, p);
  return check_launch("assign_kernel");
}

}  // extern "C"
