/*
 * ref_physics_driver.cpp -- TEST INFRASTRUCTURE ONLY (never linked into the product).
 *
 * Drives the reference's own Additive<double> with Minimizer::physics() and dumps the particle
 * positions after every physics step and the audio: what tests/golden/physics_ref.npz was made with
 * (make_golden_physics.py compiles it into oracle/_ref/ with oracle/Makefile's REF_CXXFLAGS and
 * stubs).  No line of the reference is copied here; a subclass reads the protected `particles`.
 *
 * <cstring> comes first and nothing else: the reference's headers then see exactly the standard
 * declarations their own includes give them, so particle.h's unqualified abs() binds the way this
 * toolchain binds it (the integer overload: the HZ_GRAV_TRUNC law).
 *
 *   ref_physics_driver <case file> <output file>
 *
 * Case file (whitespace-separated; floating-point values as C hex floats):
 *   V O decay harmonicity k period
 *   run L | ev KIND A B | end          KIND 0 makenote(A, B), 1 endnote(A)
 * per sample: y = a(); if (T >= period && T % period == 0) a.physics(); a.tick(); T++
 * (period 2 is the schedule of tests/additive.cpp's Metro<double>(24000)).
 * Output, raw little-endian float64: the samples, then V*O positions per physics step.
 */
#include <cstring>

#include "additive.h"

#include <cstdio>
#include <string>

using namespace soundmath;

struct Probe : Additive<double>
{
	using Additive<double>::Additive;
	double at(long i) { return particles[i](); }
};

static FILE* fin;

static void fail(const char* what)
{
	fprintf(stderr, "ref_physics_driver: %s\n", what);
	exit(2);
}

static std::string tok()
{
	char b[128];
	if (fscanf(fin, "%127s", b) != 1) fail("unexpected end of case file");
	return b;
}

static double num()
{
	std::string s = tok();
	char* e;
	double v = strtod(s.c_str(), &e);
	if (*e || e == s.c_str()) fail("bad number");
	return v;
}

int main(int argc, char** argv)
{
	if (argc != 3) fail("usage: ref_physics_driver <case file> <output file>");
	fin = fopen(argv[1], "r");
	if (!fin) fail("cannot open the case file");
	long V = (long)num(), O = (long)num();
	double decay = num(), harm = num(), k = num();
	long period = (long)num(), T = 0;
	Probe a(&cycle, V, O, decay, harm, k);
	std::vector<double> audio, track;
	for (;;)
	{
		std::string s = tok();
		if (s == "end") break;
		if (s == "run")
		{
			long L = (long)num();
			for (long t = 0; t < L; t++, T++)
			{
				audio.push_back(a());
				if (period > 0 && T >= period && T % period == 0)
				{
					a.physics();
					for (long i = 0; i < V * O; i++) track.push_back(a.at(i));
				}
				a.tick();
			}
		}
		else if (s == "ev")
		{
			long kind = (long)num();
			double A = num(), B = num();
			if (kind == 0) a.makenote(A, B);
			else if (kind == 1) a.endnote(A);
			else fail("unknown event");
		}
		else fail("unknown operation");
	}
	fclose(fin);
	FILE* fo = fopen(argv[2], "wb");
	if (!fo) fail("cannot open the output file");
	audio.insert(audio.end(), track.begin(), track.end());
	if (fwrite(audio.data(), sizeof(double), audio.size(), fo) != audio.size()) fail("short write");
	if (fclose(fo)) fail("short write");
	return 0;
}
