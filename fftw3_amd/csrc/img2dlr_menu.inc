/* img2dlr_menu.inc -- the (n0, n1) real image sizes of img2dlr_kernel / img2dlc_kernel (pass2dlr.hpp): X(rows, real
   columns).  Every ordered pair over {16, 32, 40, 48, 64} with at least one extent above 32 (all n1 are even).  An
   entry whose kernel spills or has a private segment in either direction leaves (profiles/img2dlr_codeobj.txt: none
   does), and so does one whose one-trip plan did not measure faster than the axis-by-axis plan in both directions by
   more than the round-to-round spread (profiles/img2dlr.txt: none; 5.1 ... 21.7 x at a spread of at most 5.9 %, all 21
   stay). */
X(16, 40) X(16, 48) X(16, 64)
X(32, 40) X(32, 48) X(32, 64)
X(40, 16) X(40, 32) X(40, 40) X(40, 48) X(40, 64)
X(48, 16) X(48, 32) X(48, 40) X(48, 48) X(48, 64)
X(64, 16) X(64, 32) X(64, 40) X(64, 48) X(64, 64)
