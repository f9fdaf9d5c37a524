// Prints the marching-tetrahedra case table of rc_iso_table.h (built by `make isocheck` for the CPU under
// AddressSanitizer + UBSan); tests/test_iso_table.py compares every entry with the rule restated in Python.
//   vert <k> <corner code of v0..v3>
//   edge <k> <pair index> <owner corner code> <edge number>
//   case <k> <mask> <triangles> <flip> <pair index of corner 0..2 of triangle 0, then of triangle 1> <the same as vref>
#include <stdio.h>

#include "rc_iso_table.h"

int main() {
  const RcIsoTables& T = kRcIso;
  for (int k = 0; k < 6; ++k) printf("vert %d %d %d %d %d\n", k, T.vert[k][0], T.vert[k][1], T.vert[k][2], T.vert[k][3]);
  for (int k = 0; k < 6; ++k)
    for (int e = 0; e < 6; ++e) printf("edge %d %d %d %d\n", k, e, T.owner[k][e], T.edge[k][e]);
  for (int k = 0; k < 6; ++k)
    for (int m = 0; m < 16; ++m) {
      printf("case %d %d %d %d", k, m, T.ntri[k][m], T.flip[k][m]);
      for (int t = 0; t < 2; ++t)
        for (int c = 0; c < 3; ++c) printf(" %d", T.tri[k][m][t][c]);
      for (int t = 0; t < 2; ++t)
        for (int c = 0; c < 3; ++c) printf(" %d", T.vref[k][m][t][c]);
      printf("\n");
    }
  return 0;
}
