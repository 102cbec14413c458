/* img2dl_menu.inc -- the (n0, n1) image sizes of img2dl_kernel (pass2dl.hpp): X(rows, columns).  Every ordered pair over
   {16, 32, 40, 48, 64} with at least one extent above 32; an entry whose kernel spills (profiles/img2dl_codeobj.txt) is dropped,
   and so is one whose one-trip plan measured no faster than the two-trip plan (profiles/img2dl.txt). */
X(16, 40) X(16, 48) X(16, 64)
X(32, 40) X(32, 48) X(32, 64)
X(40, 16) X(40, 32) X(40, 40) X(40, 48) X(40, 64)
X(48, 16) X(48, 32) X(48, 40) X(48, 48) X(48, 64)
X(64, 16) X(64, 32) X(64, 40) X(64, 48) X(64, 64)
