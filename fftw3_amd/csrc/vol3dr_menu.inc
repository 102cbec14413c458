/* vol3dr_menu.inc -- the (n0, n1, n2) real volume sizes of vol3dr_kernel / vol3dc_kernel (pass3dr.hpp): X(n0, n1, n2),
   row-major, n2 reals fastest and even.  One menu for both directions.  The candidates were the 68 triples of
   vol3d_menu.inc with an even n2, 32 x 32 x 8 (the real layouts differ from the complex one that had no two-way
   padding; they have one), and 5 x 5 x 10 and 15 x 15 x 6 for the path of odd extents (no self-paired plane n0 / 2, an
   odd number of row pairs).  Left: 16 x 4 x 4 (r2c) and 32 x 4 x 4 (both directions), for which the search of
   tools/perf/vol3dr_codeobj.py found no LDS padding (row padding up to 3, plane padding up to 40 doubles) that keeps
   every access pattern two-way at the tile their limits give.  No kernel spills or has a private segment
   (profiles/vol3dr_codeobj.txt), and every remaining triple measured faster than its axis-by-axis plan in both
   directions by more than the two ranges together (profiles/vol3dr.txt), so the other 69 stay. */
X(4, 4, 4) X(4, 4, 8) X(4, 4, 16) X(4, 4, 32) X(4, 8, 4) X(4, 8, 8) X(4, 8, 16) X(4, 8, 32) X(4, 16, 4) X(4, 16, 8) X(4, 16, 16) X(4, 16, 32) X(4, 32, 4) X(4, 32, 8) X(4, 32, 16) X(4, 32, 32)
X(8, 4, 4) X(8, 4, 8) X(8, 4, 16) X(8, 4, 32) X(8, 8, 4) X(8, 8, 8) X(8, 8, 16) X(8, 8, 32) X(8, 16, 4) X(8, 16, 8) X(8, 16, 16) X(8, 16, 32) X(8, 32, 4) X(8, 32, 8) X(8, 32, 16) X(8, 32, 32)
X(16, 4, 8) X(16, 4, 16) X(16, 4, 32) X(16, 8, 4) X(16, 8, 8) X(16, 8, 16) X(16, 8, 32) X(16, 16, 4) X(16, 16, 8) X(16, 16, 16) X(16, 16, 32) X(16, 32, 4) X(16, 32, 8) X(16, 32, 16)
X(32, 4, 8) X(32, 4, 16) X(32, 4, 32) X(32, 8, 4) X(32, 8, 8) X(32, 8, 16) X(32, 8, 32) X(32, 16, 4) X(32, 16, 8) X(32, 16, 16) X(32, 32, 4) X(32, 32, 8)
X(6, 6, 6) X(10, 10, 10) X(12, 12, 12) X(5, 5, 10) X(15, 15, 6)
X(6, 10, 12) X(6, 12, 10) X(10, 6, 12) X(10, 12, 6) X(12, 6, 10) X(12, 10, 6)
