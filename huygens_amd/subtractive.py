"""Subtractive<double, N> over the HIP engine.

Mirrors soundmath::Subtractive<T, N> (src/subtractive.h:15-101, the MIMO variant; note API and
physics() from Minimizer, src/minimizer.h:61-187): voices x overtones x channels two-pole
resonators (src/filter.h) retuned from the particle positions.  process(x) ==
n x {out[:, t] = operator()(x[:, t]); if (T >= period and T % period == 0) physics(); tick(); T++}
on the GPU.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from ._lib import HZ_GRAV_FABS as GRAV_FABS
from ._lib import HZ_GRAV_TRUNC as GRAV_TRUNC
from ._lib import check, dptr, load

__all__ = ["Subtractive", "GRAV_TRUNC", "GRAV_FABS"]


class Subtractive:
    def __init__(self, voices: int, overtones: int, decay: float, resonance: float = 0.99999,
                 harmonicity: float = 1.0, k: float = 0.1, channels: int = 2, device: int = 0):
        lib = load()
        h = C.c_void_p()
        check(lib.hz_sub_create(voices, overtones, channels, decay, resonance, harmonicity, k, device, C.byref(h)))
        self._h, self._lib = h, lib
        self.voices, self.overtones, self.channels = voices, overtones, channels

    def close(self):
        if getattr(self, "_h", None):
            self._lib.hz_sub_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def request(self, fundamental: float, amplitude: float = 0.0) -> int:
        v = C.c_int()
        check(self._lib.hz_sub_request(self._h, fundamental, amplitude, C.byref(v)))
        return v.value

    def release(self, voice: int):
        check(self._lib.hz_sub_release(self._h, voice))

    def makenote(self, pitch: float, amplitude: float) -> int:
        v = C.c_int()
        check(self._lib.hz_sub_makenote(self._h, pitch, amplitude, C.byref(v)))
        return v.value

    def endnote(self, pitch: float):
        check(self._lib.hz_sub_endnote(self._h, pitch))

    # ---- Minimizer::physics(); `law` is GRAV_TRUNC or GRAV_FABS, no default
    def physics_every(self, period: int, law: int):
        """A physics() step at every sample T >= period with T % period == 0, T counted from this
        call; period 0 switches it off."""
        check(self._lib.hz_sub_physics_every(self._h, period, law))

    def physics(self, law: int):
        """One physics() step now; the next tick reads the moved positions."""
        check(self._lib.hz_sub_physics(self._h, law))

    def process(self, x) -> np.ndarray:
        """x [channels][n] (or [n] with one channel) -> the same shape."""
        x = np.ascontiguousarray(x, dtype=np.float64)
        shape = x.shape
        x2 = x.reshape(self.channels, -1)
        out = np.zeros_like(x2)
        if x2.shape[1]:
            check(self._lib.hz_sub_process(self._h, dptr(x2), dptr(out), x2.shape[1]))
        return out.reshape(shape)

    def process_device(self, in_ptr: int, out_ptr: int, n: int):
        """Device pointers ([channels][n] each), asynchronous on the handle's stream."""
        check(self._lib.hz_sub_process_device(self._h, C.c_void_p(in_ptr), C.c_void_p(out_ptr), n))

    def peek(self, x) -> np.ndarray:
        """operator()(x[channels]) without tick()."""
        x = np.ascontiguousarray(x, dtype=np.float64).reshape(self.channels)
        out = np.zeros(self.channels)
        check(self._lib.hz_sub_peek(self._h, dptr(x), dptr(out)))
        return out

    def positions(self) -> np.ndarray:
        """particles[v * overtones + j]() for every particle, [voices * overtones]."""
        out = np.zeros(self.voices * self.overtones)
        check(self._lib.hz_sub_positions(self._h, dptr(out)))
        return out

    def amplitudes(self) -> np.ndarray:
        out = np.zeros(self.voices)
        check(self._lib.hz_sub_amplitudes(self._h, dptr(out)))
        return out

    def set_stream(self, stream_ptr: int | None):
        check(self._lib.hz_sub_set_stream(self._h, C.c_void_p(stream_ptr or 0)))

    def tune_physics(self, single_group_max: int = 0, tile: int = 0):
        check(self._lib.hz_sub_tune_physics(self._h, single_group_max, tile))

    def profile(self, enable: bool):
        check(self._lib.hz_sub_profile(self._h, 1 if enable else 0))

    def profile_read(self):
        """(physics, coefficient, resonator, reduce) kernel milliseconds since profile(True)."""
        ms = [C.c_double() for _ in range(4)]
        check(self._lib.hz_sub_profile_read(self._h, *[C.byref(m) for m in ms]))
        return tuple(m.value for m in ms)
