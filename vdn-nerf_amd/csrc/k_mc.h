// Marching cubes as PyMCubes numbers it: the per-cell rules shared by the dense entries (mesh.hip: vdn_mesh_mc_*) and the
// brick-sparse ones (mesh_sparse.hip: vdn_mesh_sparse_*). Both walk the same cells of the same lattice and differ only in where a
// cell's eight values and its slot in the per-cell arrays live, so everything that decides a case, a vertex or an index is here.
//
// The library the reference calls (renderer.py:36) walks the cells sequentially, x-major with z innermost, gives every cut lattice
// edge ONE vertex - created by the first visited cell that contains the edge - and numbers vertices in creation order. In parallel
// form: the count pass stores each cell's case, the number of vertices it creates and its triangle count; the caller's exclusive
// prefix sums over cells in visiting order ARE the sequential numbering; the emit pass writes each cell's vertices at its offset in
// the library's in-cell creation order and resolves a triangle corner on edge e through the cell that owns e: offset[owner] + the
// rank of e among the vertices the owner creates.
#pragma once
#include "mc_tables.h"

namespace vdn {

static __device__ __constant__ unsigned char kMcCorner[8][3] = {{0, 0, 0}, {1, 0, 0}, {1, 1, 0}, {0, 1, 0}, {0, 0, 1}, {1, 0, 1}, {1, 1, 1}, {0, 1, 1}};
static __device__ __constant__ unsigned char kMcEdge[12][2] = {{0, 1}, {1, 2}, {2, 3}, {3, 0}, {4, 5}, {5, 6}, {6, 7}, {7, 4}, {0, 4}, {1, 5}, {2, 6}, {3, 7}};
// in-cell creation order (marchingcubes.h: 0x040, 0x020, 0x400, then the shared edges where no earlier cell exists)
static __device__ __constant__ unsigned char kMcOrder[12] = {6, 5, 10, 0, 1, 2, 3, 4, 7, 8, 9, 11};

// does cell (i, j, k) create the vertex of its edge e (i.e. is it the first visited cell that contains that lattice edge)?
__device__ inline bool mc_creates(int e, int i, int j, int k) {
    switch (e) {
        case 6: case 5: case 10: return true;
        case 0: return j == 0 && k == 0;
        case 1: case 2: return k == 0;
        case 3: return i == 0 && k == 0;
        case 4: case 9: return j == 0;
        case 7: case 11: return i == 0;
        default: return i == 0 && j == 0;      // 8
    }
}
__device__ inline int mc_edge_mask(int cube) {
    int m = 0;
#pragma unroll
    for (int e = 0; e < 12; ++e)
        if (((cube >> kMcEdge[e][0]) ^ (cube >> kMcEdge[e][1])) & 1) m |= 1 << e;
    return m;
}
// marchingcubes.h: `if(v[m] <= isovalue) cubeindex |= 1<<m`, in double
__device__ inline bool mc_corner_set(float f, double isovalue) { return (double)f <= isovalue; }

// the vertices cell (i, j, k) creates among its cut edges, and the triangles of its case
__device__ inline int mc_count_verts(int edges, int i, int j, int k) {
    int nv = 0;
#pragma unroll
    for (int e = 0; e < 12; ++e)
        if (((edges >> e) & 1) && mc_creates(e, i, j, k)) ++nv;
    return nv;
}
__device__ inline int mc_count_tris(int cube) {
    int nt = 0;
    for (int t = 0; t < 16 && kMcTri[cube][t] >= 0; t += 3) ++nt;
    return nt;
}

// the lattice axis edge e runs along
__device__ inline int mc_edge_axis(int e) {
    const int ca = kMcEdge[e][0], cb = kMcEdge[e][1];
    return kMcCorner[ca][0] != kMcCorner[cb][0] ? 0 : (kMcCorner[ca][1] != kMcCorner[cb][1] ? 1 : 2);
}

// the vertex on edge e of cell (i, j, k) whose corner values are v[8]: interpolated FROM corner a TO corner b of the edge, in double:
// (x_b - x_a) * (isovalue - f_a) / (f_b - f_a) + x_a, the midpoint when f_a == f_b  (mc_isovalue_interpolation)
__device__ inline void mc_vertex(int e, int i, int j, int k, const double* v, double isovalue, double* p) {
    const int ca = kMcEdge[e][0], cb = kMcEdge[e][1];
    p[0] = (double)(i + kMcCorner[ca][0]); p[1] = (double)(j + kMcCorner[ca][1]); p[2] = (double)(k + kMcCorner[ca][2]);
    const int ax = mc_edge_axis(e);
    const double x1 = p[ax], x2 = (double)((ax == 0 ? i : (ax == 1 ? j : k)) + kMcCorner[cb][ax]);
    const double f1 = v[ca], f2 = v[cb];
    p[ax] = f2 == f1 ? (x2 + x1) / 2.0 : (x2 - x1) * (isovalue - f1) / (f2 - f1) + x1;
}

// the cell that owns (creates the vertex of) edge e of cell (i, j, k), and the owner's own number for that edge. (lx, ly, lz) is the
// lattice position of the edge's lower end, ax its axis: both are what the missed-edge check of the sparse path walks too.
struct McOwner {
    int i, j, k, e;
    int lx, ly, lz, ax;
};
__device__ inline McOwner mc_owner(int e, int i, int j, int k) {
    McOwner o;
    const int ca = kMcEdge[e][0], cb = kMcEdge[e][1];
    o.ax = mc_edge_axis(e);
    o.lx = i + min(kMcCorner[ca][0], kMcCorner[cb][0]); o.ly = j + min(kMcCorner[ca][1], kMcCorner[cb][1]); o.lz = k + min(kMcCorner[ca][2], kMcCorner[cb][2]);
    // along the edge's axis the cell index is fixed; across it, the lower neighbour where one exists
    o.i = o.ax == 0 ? o.lx : max(o.lx - 1, 0); o.j = o.ax == 1 ? o.ly : max(o.ly - 1, 0); o.k = o.ax == 2 ? o.lz : max(o.lz - 1, 0);
    const int dx = o.lx - o.i, dy = o.ly - o.j, dz = o.lz - o.k;
    if (o.ax == 0) o.e = dy == 0 ? (dz == 0 ? 0 : 4) : (dz == 0 ? 2 : 6);
    else if (o.ax == 1) o.e = dx == 0 ? (dz == 0 ? 3 : 7) : (dz == 0 ? 1 : 5);
    else o.e = dx == 0 ? (dy == 0 ? 8 : 11) : (dy == 0 ? 9 : 10);
    return o;
}
// the rank of the owner's edge oe among the vertices the owner (case edges `oedges`) creates
__device__ inline int mc_rank(int oedges, int oe, int oi, int oj, int ok) {
    int rank = 0;
    for (int o = 0; o < 12 && kMcOrder[o] != oe; ++o) {
        const int e2 = kMcOrder[o];
        if (((oedges >> e2) & 1) && mc_creates(e2, oi, oj, ok)) ++rank;
    }
    return rank;
}

}  // namespace vdn
