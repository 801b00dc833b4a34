// transpose_host_proc.cpp -- the transposer's scatter loop as a host processor with C linkage, for
// scripts/transpose_timing.py: the host-processor path (forward launch, copy out, this loop, copy
// in, inverse launch, one synchronisation per block) is what HZ_PROC_TRANSPOSE replaces.  Built as
// a shared object by the script; the frame size and ratio are set before the first frame.
#include <cstring>

static int g_n = 0;
static double g_ratio = 2.0;

extern "C" void transpose_host_setup(int n, double ratio) {
    g_n = n;
    g_ratio = ratio;
}

extern "C" int transpose_host_proc(const double* in, double* out) {   // interleaved complex
    const int n = g_n;
    std::memset(out, 0, sizeof(double) * 2 * n);
    for (int i = 0; i < n / 2; ++i) {
        const int ix = (int)(i * g_ratio);
        if (ix < n) {
            out[2 * ix] += in[2 * i];
            out[2 * ix + 1] += in[2 * i + 1];
        }
    }
    for (int i = n / 2; i < n; ++i) {
        out[2 * i] = out[2 * (n - i)];
        out[2 * i + 1] = out[2 * (n - i) + 1];
    }
    return 0;
}
