/* img2dr_menu.inc -- the (n0, n1) real image sizes of img2dr_kernel / img2dc_kernel (pass2dr.hpp): X(rows, real columns).
   Every ordered pair over {4, 5, 6, 8, 10, 12, 15, 16, 20, 24, 25, 30, 32} with an even n1.  An entry whose kernel spills
   leaves (profiles/img2dr_codeobj.txt: none does), and so does one whose one-trip plan did not measure faster than the
   three-trip plan in both directions (profiles/img2dr.txt: none; all 130 stay). */
X(4, 4) X(4, 6) X(4, 8) X(4, 10) X(4, 12) X(4, 16) X(4, 20) X(4, 24) X(4, 30) X(4, 32)
X(5, 4) X(5, 6) X(5, 8) X(5, 10) X(5, 12) X(5, 16) X(5, 20) X(5, 24) X(5, 30) X(5, 32)
X(6, 4) X(6, 6) X(6, 8) X(6, 10) X(6, 12) X(6, 16) X(6, 20) X(6, 24) X(6, 30) X(6, 32)
X(8, 4) X(8, 6) X(8, 8) X(8, 10) X(8, 12) X(8, 16) X(8, 20) X(8, 24) X(8, 30) X(8, 32)
X(10, 4) X(10, 6) X(10, 8) X(10, 10) X(10, 12) X(10, 16) X(10, 20) X(10, 24) X(10, 30) X(10, 32)
X(12, 4) X(12, 6) X(12, 8) X(12, 10) X(12, 12) X(12, 16) X(12, 20) X(12, 24) X(12, 30) X(12, 32)
X(15, 4) X(15, 6) X(15, 8) X(15, 10) X(15, 12) X(15, 16) X(15, 20) X(15, 24) X(15, 30) X(15, 32)
X(16, 4) X(16, 6) X(16, 8) X(16, 10) X(16, 12) X(16, 16) X(16, 20) X(16, 24) X(16, 30) X(16, 32)
X(20, 4) X(20, 6) X(20, 8) X(20, 10) X(20, 12) X(20, 16) X(20, 20) X(20, 24) X(20, 30) X(20, 32)
X(24, 4) X(24, 6) X(24, 8) X(24, 10) X(24, 12) X(24, 16) X(24, 20) X(24, 24) X(24, 30) X(24, 32)
X(25, 4) X(25, 6) X(25, 8) X(25, 10) X(25, 12) X(25, 16) X(25, 20) X(25, 24) X(25, 30) X(25, 32)
X(30, 4) X(30, 6) X(30, 8) X(30, 10) X(30, 12) X(30, 16) X(30, 20) X(30, 24) X(30, 30) X(30, 32)
X(32, 4) X(32, 6) X(32, 8) X(32, 10) X(32, 12) X(32, 16) X(32, 20) X(32, 24) X(32, 30) X(32, 32)
