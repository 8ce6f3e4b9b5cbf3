// Brick-sparse marching cubes (vdn_mesh_sparse_*: include/vdn_render.h; vdn_hip/mesh.py: marching_cubes_sparse).
// The (R-1)^3 cells of the lattice are cut into bricks of B^3 cells; the caller keeps the bricks the surface can pass through
// ("active") and evaluates the field only at their nodes, one (B+1)^3 value block per active brick. The kernels here triangulate
// the cells of the active bricks and produce the arrays the dense entries (mesh.hip: vdn_mesh_mc_*) produce on the full lattice,
// element for element: the per-cell rules are k_mc.h's, and a cell's slot in the per-cell arrays is its rank among the active
// cells in ascending global cell number, so the caller's prefix sums give the dense offsets (skipped cells contribute zero).
//
// One thread per (active brick, local cell). Gather-shaped, HBM / L2 bound integer work: 8 value loads per cell from the brick's
// own block (neighbouring threads share them through L1), three small table reads for the cell's rank.
#include <hip/hip_runtime.h>
#include <cstdint>
#include "vdn_render.h"
#include "k_mc.h"

namespace vdn {

// brick coordinates of a brick number, and the brick of a cell
struct Brick {
    int bi, bj, bk;
};
__device__ inline Brick brick_of_number(int b, int nb) {
    Brick q;
    q.bk = b % nb; q.bj = (b / nb) % nb; q.bi = b / (nb * nb);
    return q;
}

// node coordinates of the active bricks' value blocks: point p = slot * E^3 + ((a * E + b) * E + c), E = B + 1, is lattice node
// (bi B + a, bj B + b, bk B + c) of brick active[slot], each index clamped to R - 1 (a partial last brick repeats its last node:
// those values are never read)
__global__ void mesh_sparse_nodes_kernel(VdnMeshSparseNodesArgs a) {
    const long t = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= a.n_points) return;
    const long p = a.first + t;
    const int E = a.brick + 1, E3 = E * E * E;
    const int slot = (int)(p / E3), l = (int)(p % E3);
    const Brick q = brick_of_number(min(max(a.active[slot], 0), a.nb * a.nb * a.nb - 1), a.nb);
    const int ix = min(q.bi * a.brick + l / (E * E), a.R - 1);
    const int iy = min(q.bj * a.brick + (l / E) % E, a.R - 1);
    const int iz = min(q.bk * a.brick + l % E, a.R - 1);
    a.points[t * 3 + 0] = a.X[ix];
    a.points[t * 3 + 1] = a.Y[iy];
    a.points[t * 3 + 2] = a.Z[iz];
}

// rank of cell (i, j, k) of an ACTIVE brick among the active cells in ascending global cell number (i * n + j) * n + k:
// cell_base[brick] counts the active cells of the i-planes before the brick's first plane, of the j-columns of that plane before
// the brick's first column and of the bricks below it in its own column; one more i-plane inside the brick adds row_cells[bi],
// one more j-column col_cells[bi][bj], one more cell along z one.
__device__ inline long sparse_rank(const VdnMeshSparseArgs& a, int i, int j, int k) {
    const int B = a.brick, bi = i / B, bj = j / B, bk = k / B;
    return (long)a.cell_base[(bi * a.nb + bj) * a.nb + bk] + (long)(i - bi * B) * a.row_cells[bi] + (long)(j - bj * B) * a.col_cells[bi * a.nb + bj] + (k - bk * B);
}
__device__ inline bool sparse_cell_active(const VdnMeshSparseArgs& a, int i, int j, int k) {
    const int B = a.brick;
    return a.brick_map[((i / B) * a.nb + j / B) * a.nb + k / B] >= 0;
}

// this thread's cell: false outside the lattice (partial bricks) or past the last active brick
__device__ inline bool sparse_cell(const VdnMeshSparseArgs& a, int* slot, int* i, int* j, int* k, int* di, int* dj, int* dk) {
    const long t = (long)blockIdx.x * blockDim.x + threadIdx.x;
    const int B = a.brick, B3 = B * B * B;
    if (t >= (long)a.A * B3) return false;
    *slot = (int)(t / B3);
    const int l = (int)(t % B3);
    *di = l / (B * B); *dj = (l / B) % B; *dk = l % B;
    const int b = a.active[*slot];
    if (b < 0 || b >= a.nb * a.nb * a.nb) return false;
    const Brick q = brick_of_number(b, a.nb);
    *i = q.bi * B + *di; *j = q.bj * B + *dj; *k = q.bk * B + *dk;
    const int n = a.R - 1;
    return *i < n && *j < n && *k < n;
}

__device__ inline int sparse_case(const VdnMeshSparseArgs& a, int slot, int di, int dj, int dk, double* v) {
    const int E = a.brick + 1;
    const float* blk = a.values + (long)slot * (E * E * E);
    int cube = 0;
#pragma unroll
    for (int m = 0; m < 8; ++m) {
        const float f = blk[((di + kMcCorner[m][0]) * E + (dj + kMcCorner[m][1])) * E + (dk + kMcCorner[m][2])];
        if (v != nullptr) v[m] = (double)f;
        if (mc_corner_set(f, a.isovalue)) cube |= 1 << m;
    }
    return cube;
}

// count pass + the missed-edge check: for every cut lattice edge of an active cell, every existing cell that contains the edge must
// lie in an active brick (otherwise the surface leaves the evaluated region there: the caller's bound was too small)
__global__ void mesh_sparse_count_kernel(VdnMeshSparseArgs a) {
    int slot, i, j, k, di, dj, dk;
    if (!sparse_cell(a, &slot, &i, &j, &k, &di, &dj, &dk)) return;
    const long c = sparse_rank(a, i, j, k);
    if (c < 0 || c >= a.n_cells) return;                  // (tables that do not describe `active`: write nothing)
    const int cube = sparse_case(a, slot, di, dj, dk, nullptr);
    const int edges = mc_edge_mask(cube);
    a.cube_case[c] = (unsigned char)cube;
    a.n_verts[c] = mc_count_verts(edges, i, j, k);
    a.n_tris[c] = mc_count_tris(cube);
    if (edges == 0) return;
    const int n = a.R - 1;
    int missed = 0;
    for (int e = 0; e < 12; ++e) {
        if (!((edges >> e) & 1)) continue;
        const McOwner o = mc_owner(e, i, j, k);
        // the up to four cells round the edge: the index along its axis is fixed, across it l - 1 and l where they exist
        for (int s = 0; s < 4; ++s) {
            const int du = s & 1, dv = s >> 1;
            const int ci = o.ax == 0 ? o.lx : o.lx - du;
            const int cj = o.ax == 1 ? o.ly : o.ly - (o.ax == 0 ? du : dv);
            const int ck = o.ax == 2 ? o.lz : o.lz - dv;
            if (ci < 0 || cj < 0 || ck < 0 || ci >= n || cj >= n || ck >= n) continue;
            if (!sparse_cell_active(a, ci, cj, ck)) ++missed;
        }
    }
    if (missed != 0) atomicAdd(a.missed, missed);
}

__global__ void mesh_sparse_emit_kernel(VdnMeshSparseArgs a) {
    int slot, i, j, k, di, dj, dk;
    if (!sparse_cell(a, &slot, &i, &j, &k, &di, &dj, &dk)) return;
    const long c = sparse_rank(a, i, j, k);
    if (c < 0 || c >= a.n_cells) return;
    const int cube = a.cube_case[c];
    const int edges = mc_edge_mask(cube);
    if (edges == 0) return;
    double v[8];
    sparse_case(a, slot, di, dj, dk, v);
    // this cell's own vertices, in the library's creation order
    long vo = a.vert_offsets[c];
    for (int o = 0; o < 12; ++o) {
        const int e = kMcOrder[o];
        if (!((edges >> e) & 1) || !mc_creates(e, i, j, k)) continue;
        if (vo >= a.V) break;
        double p[3];
        mc_vertex(e, i, j, k, v, a.isovalue, p);
        a.vertices[vo * 3 + 0] = p[0]; a.vertices[vo * 3 + 1] = p[1]; a.vertices[vo * 3 + 2] = p[2];
        ++vo;
    }
    // triangles, through the owner cell and the brick map. An owner in a dropped brick was counted as a missed edge by the count
    // pass (the caller raises): no index is written and nothing is read for it.
    const long to = a.tri_offsets[c];
    for (int t = 0; t < 16 && kMcTri[cube][t] >= 0; ++t) {
        const McOwner o = mc_owner(kMcTri[cube][t], i, j, k);
        if (!sparse_cell_active(a, o.i, o.j, o.k)) continue;
        const long oc = sparse_rank(a, o.i, o.j, o.k);
        if (oc < 0 || oc >= a.n_cells || to + t / 3 >= a.F) continue;
        a.triangles[to * 3 + t] = a.vert_offsets[oc] + mc_rank(mc_edge_mask(a.cube_case[oc]), o.e, o.i, o.j, o.k);
    }
}

}  // namespace vdn

// sizes the 32-bit arithmetic of the kernels holds: brick numbers, points of the value blocks and cells of the active bricks
static int sparse_sizes(int R, int brick, int nb, int A) {
    if (R < 2 || brick < 1 || nb < 1 || A < 0) return -1;
    if ((long)brick * nb < (long)R - 1 || (long)brick * (nb - 1) >= (long)R - 1) return -1;         // nb = ceil((R - 1) / brick)
    const long E = (long)brick + 1;
    if (brick > 1024 || (long)nb * nb * nb >= (1L << 31) || (long)A > (long)nb * nb * nb) return -10;
    if ((long)A * E * E * E >= (1L << 31)) return -10;
    return 0;
}

extern "C" int vdn_mesh_sparse_nodes(const VdnMeshSparseNodesArgs* a, void* stream) {
    if (a == nullptr || a->X == nullptr || a->Y == nullptr || a->Z == nullptr || a->active == nullptr || a->points == nullptr) return -1;
    const int rc = sparse_sizes(a->R, a->brick, a->nb, a->A);
    if (rc != 0) return rc;
    const long E = (long)a->brick + 1;
    if (a->first < 0 || a->n_points < 1 || a->first + a->n_points > (long)a->A * E * E * E) return -1;
    hipLaunchKernelGGL(vdn::mesh_sparse_nodes_kernel, dim3((unsigned)((a->n_points + 255) / 256)), dim3(256), 0, (hipStream_t)stream, *a);
    return (int)hipGetLastError();
}

static int sparse_check(const VdnMeshSparseArgs* a) {
    if (a == nullptr || a->values == nullptr || a->active == nullptr || a->brick_map == nullptr || a->cell_base == nullptr ||
        a->col_cells == nullptr || a->row_cells == nullptr || a->cube_case == nullptr) return -1;
    const int rc = sparse_sizes(a->R, a->brick, a->nb, a->A);
    if (rc != 0) return rc;
    if (a->A < 1 || a->n_cells < 1 || a->n_cells > (long)a->A * a->brick * a->brick * a->brick) return -1;
    return 0;
}

extern "C" int vdn_mesh_sparse_count(const VdnMeshSparseArgs* a, void* stream) {
    const int rc = sparse_check(a);
    if (rc != 0) return rc;
    if (a->n_verts == nullptr || a->n_tris == nullptr || a->missed == nullptr) return -1;
    const long n = (long)a->A * a->brick * a->brick * a->brick;
    hipLaunchKernelGGL(vdn::mesh_sparse_count_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, *a);
    return (int)hipGetLastError();
}

extern "C" int vdn_mesh_sparse_emit(const VdnMeshSparseArgs* a, void* stream) {
    const int rc = sparse_check(a);
    if (rc != 0) return rc;
    if (a->vert_offsets == nullptr || a->tri_offsets == nullptr || a->vertices == nullptr || a->triangles == nullptr || a->V < 1 || a->F < 1) return -1;
    const long n = (long)a->A * a->brick * a->brick * a->brick;
    hipLaunchKernelGGL(vdn::mesh_sparse_emit_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, *a);
    return (int)hipGetLastError();
}
