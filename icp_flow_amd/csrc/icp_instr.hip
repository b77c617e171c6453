// icp_instr.hip -- the instruments of the debug variants of icp.hip (tools/dbg: the library built with -DICPFLOW_...):
// per instrument, under its #ifdef, the __device__ globals icp_pair writes, its ICPFLOW_STAMP where it has one, and the
// extern "C" accessors the tools read the globals through.  The product library defines none of them: all that is left
// is the empty ICPFLOW_STAMP.
// NOT a translation unit and not a header either: it DEFINES globals and functions, so it is a part of icp.hip's unit, included
// there once and before kabsch.hpp (the solver carries the phase stamps), and is not in build.py's SOURCES.  The library
// is built without relocatable device code, so a __device__ global is visible only in the unit that defines it -- the
// one that instantiates icp_kernel.
#pragma once
#include <hip/hip_runtime.h>

namespace icpflow {

#ifdef ICPFLOW_PHASE_TIMING
// tools/dbg/phase_timing.py: shader-clock stamps of workgroup 0
__device__ long long g_phase_stamps[16];
__device__ long long g_wave_stamps[16 * 16];   // [wave][k] of workgroup 0
__device__ int g_stamp_block;                  // the workgroup that stamps (icpflow_debug_set_stamp_block)
#define ICPFLOW_STAMP(k) do { if ((int)blockIdx.x == g_stamp_block && threadIdx.x == 0) g_phase_stamps[k] = clock64(); \
    if ((int)blockIdx.x == g_stamp_block && (threadIdx.x & 63) == 0) g_wave_stamps[(threadIdx.x >> 6) * 16 + (k)] = clock64(); } while (0)
extern "C" int icpflow_debug_set_stamp_block(int b)
{
    return (int)hipMemcpyToSymbol(HIP_SYMBOL(g_stamp_block), &b, sizeof(int));
}
extern "C" int icpflow_debug_phase_stamps(long long *out16)
{
    return (int)hipMemcpyFromSymbol(out16, HIP_SYMBOL(g_phase_stamps), sizeof(long long) * 16);
}
extern "C" int icpflow_debug_wave_stamps(long long *out256)
{
    return (int)hipMemcpyFromSymbol(out256, HIP_SYMBOL(g_wave_stamps), sizeof(long long) * 256);
}
#else
#define ICPFLOW_STAMP(k) do { } while (0)
#endif

#ifdef ICPFLOW_TAIL_CLOCK
// tools/dbg/tail_clock.py: per pair, shader clocks wave 0 spent between the block barrier and the publication of (R, T)
// (the serial tail), in the rest of the loop, and the iterations it executed; and the tail split at the phase stamps
// (accumulated in LDS by thread 0)
__device__ long long g_tail_clock[1024 * 3];
__device__ long long g_wg_wall[8192 * 4];   // per pair: wall clock (100 MHz) at entry and exit of its workgroup, HW_ID, XCC_ID
__device__ int g_unit_pair = -1;                       // pair whose per-(iteration, pass, wave) clocks are recorded (owner, no helpers)
__device__ long long g_unit_clk[64 * 8 * 16];
__device__ int g_unit_win[64 * 8 * 16 * 2];   // per (iteration, pass, wave): targets in the scanned window, lanes that searched
__device__ unsigned long long g_pair_help[1024];   // passes the pair's owner received from helpers
__device__ unsigned long long g_pair_hclk[1024 * 4];   // per pair: helper pass clocks, helper passes, helper waits (100 MHz), owner waits (100 MHz)
__device__ unsigned long long g_help_stats[8];   // helpers that joined a pair, passes the owners took from helpers, owner clocks spent waiting
__device__ long long g_tail_split[1024 * 16];
__shared__ long long g_tcSh[17];
#ifdef ICPFLOW_TAIL_SPLIT   // (each stamp costs ~200 clocks: the totals above are measured without)
#undef ICPFLOW_STAMP
#define ICPFLOW_STAMP(k) do { if (threadIdx.x == 0) { const long long t_ = clock64(); g_tcSh[k] += t_ - g_tcSh[16]; g_tcSh[16] = t_; } } while (0)
#endif
extern "C" int icpflow_debug_tail_clock(long long *out3072)
{
    return (int)hipMemcpyFromSymbol(out3072, HIP_SYMBOL(g_tail_clock), sizeof(long long) * 3072);
}
extern "C" int icpflow_debug_pair_hclk(unsigned long long *out4096, int reset)
{
    int rc = (int)hipMemcpyFromSymbol(out4096, HIP_SYMBOL(g_pair_hclk), sizeof(unsigned long long) * 4096);
    if (reset) { static unsigned long long z[4096]; rc |= (int)hipMemcpyToSymbol(HIP_SYMBOL(g_pair_hclk), z, sizeof(z)); }
    return rc;
}
extern "C" int icpflow_debug_unit_win(int *out16384)
{
    return (int)hipMemcpyFromSymbol(out16384, HIP_SYMBOL(g_unit_win), sizeof(int) * 16384);
}
extern "C" int icpflow_debug_unit_clk(long long *out8192, int pair)
{
    int rc = (int)hipMemcpyFromSymbol(out8192, HIP_SYMBOL(g_unit_clk), sizeof(long long) * 8192);
    rc |= (int)hipMemcpyToSymbol(HIP_SYMBOL(g_unit_pair), &pair, sizeof(int));
    return rc;
}
extern "C" int icpflow_debug_pair_help(unsigned long long *out1024, int reset)
{
    int rc = (int)hipMemcpyFromSymbol(out1024, HIP_SYMBOL(g_pair_help), sizeof(unsigned long long) * 1024);
    if (reset) { static unsigned long long z[1024]; rc |= (int)hipMemcpyToSymbol(HIP_SYMBOL(g_pair_help), z, sizeof(z)); }
    return rc;
}
extern "C" int icpflow_debug_wg_wall(long long *out32768)
{
    return (int)hipMemcpyFromSymbol(out32768, HIP_SYMBOL(g_wg_wall), sizeof(long long) * 32768);
}
extern "C" int icpflow_debug_help_stats(unsigned long long *out8, int reset)
{
    int rc = (int)hipMemcpyFromSymbol(out8, HIP_SYMBOL(g_help_stats), sizeof(unsigned long long) * 8);
    if (reset) { static unsigned long long z[8]; rc |= (int)hipMemcpyToSymbol(HIP_SYMBOL(g_help_stats), z, sizeof(z)); }
    return rc;
}
extern "C" int icpflow_debug_tail_split(long long *out16384)
{
    return (int)hipMemcpyFromSymbol(out16384, HIP_SYMBOL(g_tail_split), sizeof(long long) * 16384);
}
#endif

#ifdef ICPFLOW_DEBUG_SOLVE
// tools/dbg/onestep_case.py: the 18 moments, H, lambda and R of one pair's FIRST iteration
__device__ double g_dbg_solve[64];
__device__ float g_dbg_xt[4096 * 3];   // the moved points of that iteration by ORIGINAL row
__device__ int g_dbg_pair = 0;
extern "C" int icpflow_debug_solve(int pair, double *out64)
{
    if (out64 == nullptr) return (int)hipMemcpyToSymbol(HIP_SYMBOL(g_dbg_pair), &pair, sizeof(int));
    return (int)hipMemcpyFromSymbol(out64, HIP_SYMBOL(g_dbg_solve), sizeof(double) * 64);
}
extern "C" int icpflow_debug_xt(float *out12288)
{
    return (int)hipMemcpyFromSymbol(out12288, HIP_SYMBOL(g_dbg_xt), sizeof(float) * 12288);
}
#endif

#ifdef ICPFLOW_CERT_STATS
// tools/dbg/cert_stats.py: per iteration, over the whole batch: waves that ran, waves that searched, queries that searched,
// targets scanned (per wave)
__device__ unsigned long long g_cert_stats[128 * 4];
__device__ unsigned long long g_probe_stats[128 * 2];   // probes, conclusive probes
__device__ unsigned long long g_occ_cert[128 * 4];      // per iteration: queries without a certificate; of those, queries whose cell of the fixed cloud's grid is empty (plane 1: nothing within 0.98 h > gate); queries with certificate (B); outliers among ALL live queries by the grid
__device__ int g_stats_block = -1;                       // >= 0: only this workgroup counts
extern "C" int icpflow_debug_set_stats_block(int b)
{
    return (int)hipMemcpyToSymbol(HIP_SYMBOL(g_stats_block), &b, sizeof(int));
}
extern "C" int icpflow_debug_cert_stats(unsigned long long *out512, int reset)
{
    int rc = (int)hipMemcpyFromSymbol(out512, HIP_SYMBOL(g_cert_stats), sizeof(unsigned long long) * 512);
    rc |= (int)hipMemcpyFromSymbol(out512 + 512, HIP_SYMBOL(g_probe_stats), sizeof(unsigned long long) * 256);
    if (reset) {
        static unsigned long long zeros4[512];
        rc |= (int)hipMemcpyToSymbol(HIP_SYMBOL(g_occ_cert), zeros4, sizeof(zeros4));
        static unsigned long long zeros[512];
        rc |= (int)hipMemcpyToSymbol(HIP_SYMBOL(g_cert_stats), zeros, sizeof(zeros));
        rc |= (int)hipMemcpyToSymbol(HIP_SYMBOL(g_probe_stats), zeros, sizeof(unsigned long long) * 256);
    }
    return rc;
}
extern "C" int icpflow_debug_occ_cert(unsigned long long *out512)
{
    return (int)hipMemcpyFromSymbol(out512, HIP_SYMBOL(g_occ_cert), sizeof(unsigned long long) * 512);
}
#endif

}  // namespace icpflow
