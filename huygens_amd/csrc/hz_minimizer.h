// hz_minimizer.h -- launchers of the device Minimizer (hz_minimizer.hip): the particle physics of
// Minimizer<T>::physics() (src/minimizer.h:61-108) and the per-sample Additive render that follows
// the moving particles.  Called from hz_additive.hip.
#pragma once

#include "hz_common.h"

namespace hz {

struct MinParams {
    int V, O;            // voices, overtones (P = V O particles)
    double G, eps;       // Gravity::strength(1 FORCE, 0.0001)
    double k0, k1;       // spring strengths: guide -> particle 0 (0.1 FORCE), particle j-1 -> j (FORCE)
    double drag;         // Particle(0.01): relaxation(0.01)
};

// `steps` physics steps.  rows: [steps + 1][P]; row 0 holds the positions on entry, row k the
// positions after step k.  v [P] velocities (updated in place), eq [P] spring equilibria,
// act [V] Minimizer::active (the mass of an active voice's particles), guide [V] guide positions.
// single_group: one workgroup runs every step in one launch (P <= 1024); else one launch per step
// with `tile` threads per workgroup.
int min_run(hipStream_t stream, const MinParams& prm, int law, int steps, bool single_group, int tile, double* rows,
            double* v, const double* eq, const double* act, const double* guide);

struct TrackArgs {
    const double* rows;   // [steps + 1][P] position rows (row k in effect after the call's k-th step)
    const double* amp;    // [n + 1][V] envelope: row t at sample t's output, row t + 1 after its tick
    const double* act;    // [V]
    const double* c;      // [P] output weights
    double* phi;          // [P] oscillator phase   (read; written when advance)
    double* f;            // [P] oscillator frequency
    double* partial;      // [groups][n_pad] group rows (add_track_groups(P) of them)
    long n, n_pad;
    long T0;              // samples since the period was set, at the call's first sample
    int period;           // 0: no step inside the call
    int P, V, O;
    double s;             // oscillator stiffness
    int advance;          // 0: operator()() only (hz_add_peek)
};

int add_track_groups(int P);
int add_track(hipStream_t stream, const TrackArgs& a);

}  // namespace hz
