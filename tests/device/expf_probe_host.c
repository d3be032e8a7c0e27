/* Host side of the expf probe (tests/test_expf.py, tests/test_gpu_expf.py), built by the Makefile
 * with exactly $(HOSTCFLAGS) into tests/build/libuhsdr_expf_probe_host.so:
 *   ulh_expf  the host build of ul_expf (uhsdr_amd/csrc/uhsdr_libm_expf.h)
 *   ulg_expf  glibc's expf, called in libm
 * as loops over arrays: a ctypes call per operand is far too slow for tens of millions of operands. */
#define _GNU_SOURCE
#include <math.h>
#include <stddef.h>
#include <stdint.h>
#include "../../uhsdr_amd/csrc/uhsdr_libm_expf.h"

/* libm's entry point through a volatile pointer: gcc then never folds a call */
static float (*volatile g_expf)(float) = expf;

void ulh_expf(const float* x, float* r, size_t n) { for (size_t i = 0; i < n; ++i) r[i] = ul_expf(x[i]); }
void ulg_expf(const float* x, float* r, size_t n) { for (size_t i = 0; i < n; ++i) r[i] = g_expf(x[i]); }
