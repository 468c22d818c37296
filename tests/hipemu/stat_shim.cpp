// stat_shim.cpp -- the BatchNorm statistics-row arithmetic of fast-depth_amd/csrc/fd_device.h (fd_stat_add / fd_stat_total), compiled with the
// emulator's flags and exposed to ctypes so that tests/test_emu_nonfinite.py can check it against exact integer / rational sums.  TEST INFRASTRUCTURE ONLY.
#include "fd_device.h"

extern "C" {
// adds partials v[0 .. n) of column c (sum `which`): partial i comes from workgroup number blk0 + i (row (blk0 + i) & (nr - 1)), as a producer launch deals them
void fd_shim_stat_add(int dir, long long *rows, int nr, int cs, int which, int c, const float *v, long n, long blk0)
{
    const fd_stat_rows d{rows, nr, cs};
    for (long i = 0; i < n; ++i) {
        if (dir == FD_STAT_FWD) fd_stat_add<FD_STAT_FWD>(d, blk0 + i, cs, which, c, v[i]);
        else fd_stat_add<FD_STAT_BWD>(d, blk0 + i, cs, which, c, v[i]);
    }
}
double fd_shim_stat_total(int dir, const long long *rows, int nr, int cs, int which, int c, int r0, int rstep)
{
    return dir == FD_STAT_FWD ? fd_stat_total<FD_STAT_FWD>(rows, nr, cs, which, c, r0, rstep) : fd_stat_total<FD_STAT_BWD>(rows, nr, cs, which, c, r0, rstep);
}
// fd_stat_table_block's form: the rows of a column dealt to RG work-items (work-item rg sums rows rg, rg + RG, ... < nr; work-items rg >= nr contribute 0),
// their doubles added in work-item order
double fd_shim_stat_total_sliced(int dir, const long long *rows, int nr, int cs, int which, int c, int RG)
{
    double s = 0.0;
    for (int rg = 0; rg < RG; ++rg) s += rg < nr ? fd_shim_stat_total(dir, rows, nr, cs, which, c, rg, RG) : 0.0;
    return s;
}
}
