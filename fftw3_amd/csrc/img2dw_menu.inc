/* img2dw_menu.inc -- the (n0, n1) image sizes of img2dw_kernel (pass2dw.hpp): X(rows, columns).  The three pairs over
   {64, 128} with an extent of 128; every entry compiles without a spill (profiles/img2dw_codeobj.txt). */
X(64, 128) X(128, 64) X(128, 128)
