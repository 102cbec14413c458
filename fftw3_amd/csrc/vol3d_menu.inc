/* vol3d_menu.inc -- the (n0, n1, n2) volume sizes of vol3d_kernel (pass3d.hpp): X(n0, n1, n2), row-major, n2 fastest.
   (a) every ordered triple over {4, 8, 16, 32} with at most 8192 elements, but for 32 x 32 x 8: no padding of its LDS
   plane inside the 72 KiB limit keeps the exchanges at two-way bank conflicts (pass3d.hpp), so it is left out;
   (b) the cubes of 5, 6, 10, 12 and 15; (c) the six orderings of 6 x 10 x 12, the triple with three different
   prime-factor butterflies.  An entry whose kernel spills or uses a private segment is dropped
   (profiles/vol3d_codeobj.txt: none does), and so
   is one whose one-trip plan does not measure faster than the axis-by-axis plan (profiles/vol3d.txt: none does). */
X(4, 4, 4) X(4, 4, 8) X(4, 4, 16) X(4, 4, 32) X(4, 8, 4) X(4, 8, 8) X(4, 8, 16) X(4, 8, 32) X(4, 16, 4) X(4, 16, 8) X(4, 16, 16) X(4, 16, 32) X(4, 32, 4) X(4, 32, 8) X(4, 32, 16) X(4, 32, 32)
X(8, 4, 4) X(8, 4, 8) X(8, 4, 16) X(8, 4, 32) X(8, 8, 4) X(8, 8, 8) X(8, 8, 16) X(8, 8, 32) X(8, 16, 4) X(8, 16, 8) X(8, 16, 16) X(8, 16, 32) X(8, 32, 4) X(8, 32, 8) X(8, 32, 16) X(8, 32, 32)
X(16, 4, 4) X(16, 4, 8) X(16, 4, 16) X(16, 4, 32) X(16, 8, 4) X(16, 8, 8) X(16, 8, 16) X(16, 8, 32) X(16, 16, 4) X(16, 16, 8) X(16, 16, 16) X(16, 16, 32) X(16, 32, 4) X(16, 32, 8) X(16, 32, 16)
X(32, 4, 4) X(32, 4, 8) X(32, 4, 16) X(32, 4, 32) X(32, 8, 4) X(32, 8, 8) X(32, 8, 16) X(32, 8, 32) X(32, 16, 4) X(32, 16, 8) X(32, 16, 16) X(32, 32, 4)
X(5, 5, 5) X(6, 6, 6) X(10, 10, 10) X(12, 12, 12) X(15, 15, 15)
X(6, 10, 12) X(6, 12, 10) X(10, 6, 12) X(10, 12, 6) X(12, 6, 10) X(12, 10, 6)
