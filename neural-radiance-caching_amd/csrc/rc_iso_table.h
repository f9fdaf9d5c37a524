// Marching tetrahedra on the Kuhn (Freudenthal) decomposition of a lattice cell (rc_isosurface): the case
// table and the rule that generates it, evaluated by the compiler.  No HIP dependency: rc_mesh.hip reads kRcIso on the
// device, isocheck.cpp prints it on the host (tests/test_iso_table.py compares every entry with the rule restated in
// Python).
//
// A corner of the cell is the code dx | dy << 1 | dz << 2 of its offset from the cell's lowest lattice point.
// Tetrahedron k = 0..5 belongs to the k-th permutation (a, b, c) of the axes in lexicographic order (xyz, xzy, yxz, yzx,
// zxy, zyx): v0 = 0, v1 = e_a, v2 = e_a + e_b, v3 = (1, 1, 1).  A tetrahedron edge (v_i, v_j), i < j, is the pair index
// 0..5 of (0,1) (0,2) (0,3) (1,2) (1,3) (2,3); it runs from the lattice point v_i, its owner, in one of the seven
// directions (1,0,0) (0,1,0) (0,0,1) (1,1,0) (1,0,1) (0,1,1) (1,1,1), numbered in this order.
// Triangles of the inside mask m (bit i: v_i inside), with E(i, j) the vertex on edge (v_i, v_j):
//   one vertex a on its own side (inside or outside), the rest b < c < d:   (E(a,b), E(a,c), E(a,d))
//   inside {a, b}, a < b, outside {c, d}, c < d:   (E(a,c), E(a,d), E(b,d)) and (E(a,c), E(b,d), E(b,c))
// then the 2nd and 3rd corner are swapped when, on the unit cell with every vertex at its edge's midpoint,
// (q1 - q0) x (q2 - q0) has a negative dot product with (centroid of the outside vertices - centroid of the inside ones).
#pragma once
#include <stdint.h>

struct RcIsoTables {
  uint8_t vert[6][4];          // corner code of v_i
  uint8_t owner[6][6];         // tetrahedron edge (pair index) -> corner code of its owner
  uint8_t edge[6][6];          // tetrahedron edge -> its number 0..6 among the owner's edges
  uint8_t ntri[6][16];         // triangles of (k, mask)
  uint8_t flip[6][16];         // 1: the rule's triangles of (k, mask) had their 2nd and 3rd corner swapped
  uint8_t tri[6][16][2][3];    // triangle t, corner c -> pair index of its edge, oriented
  uint8_t vref[6][16][2][3];   // the same corner as owner corner code | edge number << 3
};

constexpr int kRcIsoDirCode[7] = {1, 2, 4, 3, 5, 6, 7};      // edge number -> corner code of its direction

constexpr int rc_iso_pair(int i, int j) {      // pair index of the edge {v_i, v_j}
  const int a = i < j ? i : j, b = i < j ? j : i;
  return a == 0 ? b - 1 : (a == 1 ? b + 1 : 5);
}

constexpr RcIsoTables rc_iso_make_tables() {
  RcIsoTables T{};
  const int perm[6][3] = {{0, 1, 2}, {0, 2, 1}, {1, 0, 2}, {1, 2, 0}, {2, 0, 1}, {2, 1, 0}};
  const int pi[6] = {0, 0, 0, 1, 1, 2}, pj[6] = {1, 2, 3, 2, 3, 3};
  for (int k = 0; k < 6; ++k) {
    T.vert[k][0] = 0;
    T.vert[k][1] = (uint8_t)(1 << perm[k][0]);
    T.vert[k][2] = (uint8_t)((1 << perm[k][0]) | (1 << perm[k][1]));
    T.vert[k][3] = 7;
    for (int e = 0; e < 6; ++e) {
      const int from = T.vert[k][pi[e]], dir = T.vert[k][pj[e]] ^ from;
      int num = 0;
      while (kRcIsoDirCode[num] != dir) ++num;
      T.owner[k][e] = (uint8_t)from;
      T.edge[k][e] = (uint8_t)num;
    }
    for (int m = 0; m < 16; ++m) {
      int in[4] = {0, 0, 0, 0}, out[4] = {0, 0, 0, 0}, ni = 0, no = 0;
      for (int i = 0; i < 4; ++i) {
        if ((m >> i) & 1) in[ni++] = i; else out[no++] = i;
      }
      int tri[2][3][2] = {};      // triangle, corner -> (i, j)
      int nt = 0;
      if (ni == 1 || ni == 3) {
        const int a = ni == 1 ? in[0] : out[0];
        const int* rest = ni == 1 ? out : in;
        for (int c = 0; c < 3; ++c) { tri[0][c][0] = a; tri[0][c][1] = rest[c]; }
        nt = 1;
      } else if (ni == 2) {
        const int a = in[0], b = in[1], c = out[0], d = out[1];
        tri[0][0][0] = a; tri[0][0][1] = c; tri[0][1][0] = a; tri[0][1][1] = d; tri[0][2][0] = b; tri[0][2][1] = d;
        tri[1][0][0] = a; tri[1][0][1] = c; tri[1][1][0] = b; tri[1][1][1] = d; tri[1][2][0] = b; tri[1][2][1] = c;
        nt = 2;
      }
      T.ntri[k][m] = (uint8_t)nt;
      // (centroid of the outside vertices - centroid of the inside ones) * ni * no, in integers
      int w[3] = {0, 0, 0};
      for (int ax = 0; ax < 3; ++ax) {
        int so = 0, si = 0;
        for (int i = 0; i < no; ++i) so += (T.vert[k][out[i]] >> ax) & 1;
        for (int i = 0; i < ni; ++i) si += (T.vert[k][in[i]] >> ax) & 1;
        w[ax] = so * ni - si * no;
      }
      for (int t = 0; t < nt; ++t) {
        int q[3][3] = {};         // twice the midpoint of each corner's edge
        for (int c = 0; c < 3; ++c)
          for (int ax = 0; ax < 3; ++ax)
            q[c][ax] = ((T.vert[k][tri[t][c][0]] >> ax) & 1) + ((T.vert[k][tri[t][c][1]] >> ax) & 1);
        const int u[3] = {q[1][0] - q[0][0], q[1][1] - q[0][1], q[1][2] - q[0][2]};
        const int v[3] = {q[2][0] - q[0][0], q[2][1] - q[0][1], q[2][2] - q[0][2]};
        const int cr[3] = {u[1] * v[2] - u[2] * v[1], u[2] * v[0] - u[0] * v[2], u[0] * v[1] - u[1] * v[0]};
        const bool wrong = cr[0] * w[0] + cr[1] * w[1] + cr[2] * w[2] < 0;
        if (wrong) T.flip[k][m] = 1;
        for (int c = 0; c < 3; ++c) {
          const int s = wrong ? (c == 0 ? 0 : 3 - c) : c;
          const int e = rc_iso_pair(tri[t][s][0], tri[t][s][1]);
          T.tri[k][m][t][c] = (uint8_t)e;
          T.vref[k][m][t][c] = (uint8_t)(T.owner[k][e] | (T.edge[k][e] << 3));
        }
      }
    }
  }
  return T;
}

static constexpr RcIsoTables kRcIso = rc_iso_make_tables();
