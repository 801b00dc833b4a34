/*
 * hz_ref_dump.cpp -- TEST INFRASTRUCTURE ONLY (never linked into the product).
 *
 * Drives the reference's own classes, compiled from the reference's headers where they lie
 * (make -C oracle ref, REF_SRC), and dumps what they compute: the pin that tests/golden/ref_*.npz
 * and tests/test_ref_live_cpu.py hold the restatements and the kernels to.  No line of the
 * reference is copied here; the objects are used through their public members only, in the call
 * order of the reference's own tests (tests/additive.cpp, delay.cpp, granny.cpp:
 * y = obj(); obj.tick(); per sample).
 *
 *   hz_ref_dump <subcommand> <case file> <output file>
 *
 * The case file is whitespace-separated tokens: a header (per subcommand, below), then for the
 * stateful classes a stream of operations
 *   run L             L samples
 *   ev KIND I A B     one event (KIND as in the fixtures' ev_kind; I an integer, A and B values)
 *   end
 * Every floating-point value is a C hex float (strtod), so both sides see the same bits.  The
 * output file is raw little-endian float64.
 *
 * The standard headers below come first on purpose: with <math.h>/<stdlib.h>'s C++ overloads
 * declared, the reference's unqualified abs(double) is the floating one (its author's platform);
 * without them it binds ::abs(int) silently.  The static_assert keeps a toolchain that would do
 * the latter from producing a different "reference".
 */
#include <cmath>
#include <math.h>
#include <stdlib.h>
#include <cstring>
#include <vector>
#include <functional>
#include <cstdio>
#include <string>
#include <type_traits>
#include <utility>

using std::vector;

#include "oscillator.h"
#include "synth.h"
#include "sinusoids.h"
#include "additive.h"
#include "delay.h"
#include "bowl.h"
#include "granulator.h"

namespace soundmath
{
	static_assert(std::is_same<decltype(abs(0.75)), double>::value,
	              "abs(double) binds the integer overload: not the reference's arithmetic");
}

using namespace soundmath;

static FILE* fin;
static vector<double> out;

static void fail(const char* what)
{
	fprintf(stderr, "hz_ref_dump: %s\n", what);
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

static long integer()
{
	std::string s = tok();
	char* e;
	long v = strtol(s.c_str(), &e, 10);
	if (*e || e == s.c_str()) fail("bad integer");
	return v;
}

struct Op
{
	char what;   // 'r' run, 'f' fill (Bowl), 'e' event, 0 end
	long n;      // run length, or the event's kind
	long i;
	double a, b;
};

static Op next_op()
{
	Op op = {0, 0, 0, 0, 0};
	std::string s = tok();
	if (s == "run") { op.what = 'r'; op.n = integer(); }
	else if (s == "fill") { op.what = 'f'; op.n = integer(); }
	else if (s == "ev") { op.what = 'e'; op.n = integer(); op.i = integer(); op.a = num(); op.b = num(); }
	else if (s != "end") fail("unknown operation");
	return op;
}

// event kinds (tests/ref_driver.py holds the same table)
enum
{
	MAKENOTE = 0, ENDNOTE = 1, REQUEST = 2, RELEASE = 3,
	FUNDMOD = 10, DECAYMOD = 11, HARMMOD = 12,
	FREQMOD = 20, PHASEMOD = 21, RESET = 22,
	MOD_FORWARD = 30, MOD_BACK = 31, BARE_TICKS = 32,
	TRIGGER = 50
};

// header: N, then N x (name, argument)
static void scalars()
{
	long n = integer();
	for (long i = 0; i < n; i++)
	{
		std::string f = tok();
		double x = num();
		if (f == "relaxation") out.push_back(relaxation(x));
		else if (f == "mtof") out.push_back(mtof(x));
		else if (f == "ftom") out.push_back(ftom(x));
		else if (f == "dbtoa") out.push_back(dbtoa(x));
		else fail("unknown scalar function");
	}
}

// header: P, then P phases; output [8][P]
static void wave()
{
	long n = integer();
	vector<double> p(n);
	for (long i = 0; i < n; i++) p[i] = num();
	Wave<double>* all[8] = {&saw, &triangle, &square, &phasor, &cycle, &hann, &halfhann, &limiter};
	for (int w = 0; w < 8; w++)
		for (long i = 0; i < n; i++)
			out.push_back((*all[w])(p[i]));
}

template <typename O> static void oscillator_ops(O& o)
{
	for (Op op = next_op(); op.what; op = next_op())
	{
		if (op.what == 'r')
			for (long t = 0; t < op.n; t++) { out.push_back(o()); o.tick(); }
		else if (op.n == FREQMOD) o.freqmod(op.a);
		else if (op.n == PHASEMOD) o.phasemod(op.a);
		else if (op.n == RESET) o.reset(op.a);
		else fail("oscillator: unknown event");
	}
}

// header: f phi k
static void oscillator()
{
	double f = num(), phi = num(), k = num();
	Oscillator<double> o(f, phi, k);
	oscillator_ops(o);
}

static void synth()
{
	double f = num(), phi = num(), k = num();
	Synth<double> s(&cycle, f, phi, k);
	oscillator_ops(s);
}

// header: fundamental overtones decay harmonicity k
static void sinusoids()
{
	double fund = num();
	long O = integer();
	double decay = num(), harm = num(), k = num();
	Sinusoids<double> s(&cycle, fund, O, decay, harm, k);
	for (Op op = next_op(); op.what; op = next_op())
	{
		if (op.what == 'r')
			for (long t = 0; t < op.n; t++) { out.push_back(s()); s.tick(); }
		else if (op.n == FUNDMOD) s.fundmod(op.a);
		else if (op.n == DECAYMOD) s.decaymod(op.a);
		else if (op.n == HARMMOD) s.harmmod(op.a);
		else fail("sinusoids: unknown event");
	}
}

// header: voices overtones decay harmonicity k
static void additive()
{
	long V = integer(), O = integer();
	double decay = num(), harm = num(), k = num();
	Additive<double> a(&cycle, V, O, decay, harm, k);
	for (Op op = next_op(); op.what; op = next_op())
	{
		if (op.what == 'r')
			for (long t = 0; t < op.n; t++) { out.push_back(a()); a.tick(); }
		else if (op.n == MAKENOTE) a.makenote(op.a, op.b);
		else if (op.n == ENDNOTE) a.endnote(op.a);
		else if (op.n == REQUEST) a.request(op.a, op.b);
		else if (op.n == RELEASE) a.release((int)op.a);
		else fail("additive: unknown event");
	}
}

// header: lines sparsity time rows n, x[rows][n] (rows 1: one input for every line), then per line
// nf, nf x (time gain), nb, nb x (time gain).  Events: I = line * 65536 + tap.  Output [lines][n].
template <typename T> static void delay_lines()
{
	long lines = integer(), S = integer(), time = integer(), rows = integer(), n = integer();
	vector<T> x(rows * n);
	for (long i = 0; i < rows * n; i++) x[i] = (T)num();
	vector<Delay<T>*> d(lines);
	for (long l = 0; l < lines; l++)
	{
		d[l] = new Delay<T>(S, time);
		vector<std::pair<uint, T>> fwd, back;
		for (long c = integer(); c > 0; c--) { uint t = integer(); fwd.push_back({t, (T)num()}); }
		for (long c = integer(); c > 0; c--) { uint t = integer(); back.push_back({t, (T)num()}); }
		d[l]->coefficients(fwd, back);
	}
	out.assign(lines * n, 0.0);
	long pos = 0;
	for (Op op = next_op(); op.what; op = next_op())
	{
		if (op.what == 'r')
		{
			if (pos + op.n > n) fail("delay: run past the input");
			for (long t = 0; t < op.n; t++, pos++)
				for (long l = 0; l < lines; l++)
				{
					out[l * n + pos] = (*d[l])(x[(rows > 1 ? l : 0) * n + pos]);
					d[l]->tick();
				}
		}
		else if (op.n == MOD_FORWARD) d[op.i >> 16]->modulate_forward(op.i & 0xffff, {(uint)op.a, (T)op.b});
		else if (op.n == MOD_BACK) d[op.i >> 16]->modulate_back(op.i & 0xffff, {(uint)op.a, (T)op.b});
		else if (op.n == BARE_TICKS)
			for (long c = 0; c < (long)op.a; c++)
				for (long l = 0; l < lines; l++) d[l]->tick();
		else fail("delay: unknown event");
	}
	for (long l = 0; l < lines; l++) delete d[l];
}

// header: is_float, then delay_lines' header
static void delay()
{
	if (integer()) delay_lines<float>();
	else delay_lines<double>();
}

// header: overtones count, f[count] a[count] d[count]; run: operator()/tick(), fill: fill(float*)
static void bowl()
{
	long M = integer(), count = integer();
	vector<double> f(count), a(count), d(count);
	for (auto& v : f) v = num();
	for (auto& v : a) v = num();
	for (auto& v : d) v = num();
	Bowl<double> b(M, f, a, d);
	for (Op op = next_op(); op.what; op = next_op())
	{
		if (op.what == 'r')
			for (long t = 0; t < op.n; t++) { out.push_back(b()); b.tick(); }
		else if (op.what == 'f')
		{
			vector<float> buf(op.n);
			b.fill(buf.data(), op.n);
			for (float v : buf) out.push_back(v);
		}
		else if (op.n == TRIGGER) b.trigger();
		else fail("bowl: unknown event");
	}
}

// header: polyphony buffer_size n, x[n], nreq, nreq x (at offset size speed gain pan), at ascending.
// Per sample: source.write(x); y = granny(); requests at this sample; source.tick(); granny.tick().
// Output y[n], then the voice every request returned (-1: refused).
static void granulator()
{
	long P = integer(), size = integer(), n = integer();
	vector<double> x(n);
	for (auto& v : x) v = num();
	long nreq = integer();
	vector<long> at(nreq);
	vector<double> par(5 * nreq);
	for (long k = 0; k < nreq; k++)
	{
		at[k] = integer();
		for (int c = 0; c < 5; c++) par[5 * k + c] = num();
	}
	Buffer<double> source(size);
	Granulator<double> granny(&hann, &source, true, P);
	vector<double> voices(nreq, -2.0);
	long k = 0;
	for (long i = 0; i < n; i++)
	{
		source.write(x[i]);
		out.push_back(granny());
		for (; k < nreq && at[k] == i; k++)
			voices[k] = (int)granny.request(par[5 * k], par[5 * k + 1], par[5 * k + 2], par[5 * k + 3], par[5 * k + 4]);
		source.tick();
		granny.tick();
	}
	for (double v : voices) out.push_back(v);
}

int main(int argc, char** argv)
{
	if (argc != 4) fail("usage: hz_ref_dump <subcommand> <case file> <output file>");
	fin = fopen(argv[2], "r");
	if (!fin) fail("cannot open the case file");
	std::string sub = argv[1];
	if (sub == "scalars") scalars();
	else if (sub == "wave") wave();
	else if (sub == "oscillator") oscillator();
	else if (sub == "synth") synth();
	else if (sub == "sinusoids") sinusoids();
	else if (sub == "additive") additive();
	else if (sub == "delay") delay();
	else if (sub == "bowl") bowl();
	else if (sub == "granulator") granulator();
	else fail("unknown subcommand");
	fclose(fin);
	FILE* fo = fopen(argv[3], "wb");
	if (!fo) fail("cannot open the output file");
	if (!out.empty() && fwrite(out.data(), sizeof(double), out.size(), fo) != out.size()) fail("short write");
	if (fclose(fo)) fail("short write");
	return 0;
}
