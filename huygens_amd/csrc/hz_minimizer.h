// hz_minimizer.h -- launchers of the device Minimizer (hz_minimizer.hip): the particle physics of
// Minimizer<T>::physics() (src/minimizer.h:61-108) and the per-sample Additive render that follows
// the moving particles, and the host side of Minimizer's note layer (src/minimizer.h:111-187).
// Called from hz_additive.hip and hz_subtractive.hip.
#pragma once

#include <cmath>
#include <vector>

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

// Minimizer's particle constants (includes.h:34 FORCE = 50000; minimizer.h:56; particle.h:23-27, 108)
// with the instrument's spring strengths k0 (guide -> particle 0) and k1 (particle j-1 -> j)
inline MinParams min_params(int V, int O, double k0, double k1) {
    MinParams p;
    p.V = V;
    p.O = O;
    p.G = 1 * 50000;
    p.eps = 0.0001;
    p.k0 = k0;
    p.k1 = k1;
    p.drag = relaxation(0.01);
    return p;
}

// Minimizer's note layer on the host (minimizer.h:111-187): voice allocation with stealing, guides,
// particle positions and spring equilibria as request() leaves them.  The instruments derive their
// handles from it; with physics on, the device copy of `position` is the one that moves.
struct MinNotes {
    int V = 0, O = 0;
    double harmonicity = 1;
    std::vector<double> active;        // Minimizer::active (amplitude targets)
    std::vector<double> pitches;       // Minimizer::pitches
    std::vector<double> guide;         // guides[v].position
    std::vector<double> position;      // particles[v*O+j].position
    std::vector<double> equilibrium;   // springs[v*O+j].equilibrium

    void notes_init(int voices, int overtones, double harm) {
        V = voices;
        O = overtones;
        harmonicity = harm;
        active.assign(V, 0.0);
        pitches.assign(V, 0.0);
        guide.assign(V, 0.0);
        position.assign((size_t)V * O, 0.0);
        equilibrium.assign((size_t)V * O, 0.0);
    }

    static double ftom(double f) { return 69 + std::log2(f / 440.0) * 12; }
    static double mtof(double m) { return 440.0 * std::pow(2, (m - 69) / 12); }

    // request(fundamental, amplitude)  minimizer.h:111-158: the first free voice, else the voice whose
    // guide is nearest in pitch; its particles (mass 1, v = a = 0) and spring equilibria are
    // re-initialised.  Returns the voice.
    int request(double fundamental, double amplitude) {
        int voice = -1;
        for (int i = 0; i < V; ++i)
            if (!active[i]) {
                voice = i;
                break;
            }
        if (voice < 0) {  // steal the voice whose guide is nearest in pitch
            const double pitch = ftom(fundamental);
            double distance = 0;
            int nearest = -1;
            for (int i = 0; i < V; ++i) {
                double offset = pitch - guide[i];
                offset *= offset;
                if (nearest < 0 || offset < distance) {
                    nearest = i;
                    distance = offset;
                }
            }
            voice = nearest;
        }
        active[voice] = amplitude;
        guide[voice] = ftom(fundamental);
        double frequency = fundamental;
        for (int j = 0; j < O; ++j) {
            const double previous = frequency;
            frequency = fundamental * (1 + std::pow((double)j / (O - 1), harmonicity) * (O - 1));
            const double pitch = ftom(frequency);
            position[(size_t)voice * O + j] = pitch;
            equilibrium[(size_t)voice * O + j] = pitch - ftom(previous);
        }
        return voice;
    }

    // release(voice) minimizer.h:161-172 (voice < 0: all)
    void release(int voice) {
        for (int i = 0; i < V; ++i)
            if (voice < 0 || i == voice) active[i] = 0;
    }
};

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
