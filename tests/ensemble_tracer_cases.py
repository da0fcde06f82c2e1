"""Cases and helpers of the ensemble tracer tests (swmhd_ensemble_tracers_rk3_*, ShallowWaterEnsemble(tracers=...)).  The reference is
tracer_cases' (the oracle's tendency of a centre field in the A slot, numpy's update, RefModel); here are only the pitched ensemble
layout and the per-member inputs.

Layout of one field family (include/swmhd.h, Ensembles): member m's halo-padded parent at m * stride_m elements of ONE flat buffer,
rows stride_y = Nx + 2 H + PAD apart, stride_m = (Ny + 2 H) stride_y + GAP.  pack() puts the sentinel everywhere but where it is told
to put data: the pad columns, the gap after every member and -- interiors only -- every halo."""
import functools

import numpy as np

import helpers as Hh
import tracer_cases as TC

H = TC.H
PAD, GAP = 5, 37
MEMBERS, KMAX = 3, 8
SHAPES = [(3, 3), (7, 9), (TC.TX + 1, TC.TY + 1), (2 * TC.TX + 1, 9)]     # the member shapes at which the tile logic can go wrong
NPDT = {"f64": np.float64, "f32": np.float32}
COEF = dict(dt=0.013, gamma=0.37, zeta=-0.21)      # no RK3 identity that could hide a wrong operand
DTS = (0.013, 0.0071, 0.021)                       # per-member time steps of the params form


def layout(Nx, Ny):
    """(stride_y, stride_m) of the pitched ensemble."""
    sy = Nx + 2 * H + PAD
    return sy, (Ny + 2 * H) * sy + GAP


def pack(parents, Nx, Ny, dtype, halos=False):
    """The flat host buffer of one family: member m's interior (halos=True: whole parent) from parents[m] (None: nothing), the
    sentinel everywhere else."""
    sy, sm = layout(Nx, Ny)
    flat = np.full(len(parents) * sm, TC.SENTINEL, dtype=dtype)
    for m, a in enumerate(parents):
        if a is None:
            continue
        view = flat[m * sm:m * sm + (Ny + 2 * H) * sy].reshape(Ny + 2 * H, sy)
        if halos:
            view[:, :Nx + 2 * H] = a
        else:
            view[H:H + Ny, H:H + Nx] = Hh.interior(a, Nx, Ny, H, H)
    return flat


class StageInputs:
    """MEMBERS distinct states, KMAX distinct tracers and G- operands each, of one (shape, formulation, precision), halos periodic,
    with the oracle's tendency of every tracer of every member.  Built once per case (inputs) and shared: do not modify."""

    def __init__(self, O, Nx, Ny, form, sfx, rough=True, members=MEMBERS, K=KMAX, reference=True):
        t = NPDT[sfx]
        self.Nx, self.Ny, self.form, self.sfx, self.members, self.K = Nx, Ny, form, sfx, members, K
        self.dx, self.dy = float(t(TC.DX)), float(t(TC.DY))      # as the call receives them
        self.q, self.c, self.Gm, self.G = [], [], [], []
        for m in range(members):
            seed = 1000 * Nx + Ny + 7919 * m
            q = [Hh.fill_halo_periodic(a, Nx, Ny, H, H) for a in TC.state(Nx, Ny, form, seed, t, rough)]
            c = [Hh.fill_halo_periodic(a, Nx, Ny, H, H) for a in TC.tracer_fields(Nx, Ny, K, seed, t, rough)]
            gm = []
            for k in range(K):
                a = np.zeros(q[0].shape, dtype=t)
                Hh.interior(a, Nx, Ny, H, H)[...] = np.random.default_rng([seed, 200 + k]).standard_normal((Ny, Nx))
                gm.append(a)
            self.q.append(q); self.c.append(c); self.Gm.append(gm)
            if reference:
                self.G.append([TC.tracer_tendency(O, q, ck, Nx, Ny, self.dx, self.dy, form) for ck in c])

    def family(self, what, k=None, members=None, halos=False):
        """pack() of q1 | q2 | h (what = 0, 1, 2) or of tracer / G- k (what = "c" | "Gm") over the first `members` members."""
        M = self.members if members is None else members
        src = [self.q[m][what] if k is None else getattr(self, what)[m][k] for m in range(M)]
        return pack(src, self.Nx, self.Ny, NPDT[self.sfx], halos)


@functools.lru_cache(maxsize=None)
def _cached(O, Nx, Ny, form, sfx, rough):
    return StageInputs(O, Nx, Ny, form, sfx, rough)


def stage_inputs(O, Nx, Ny, form, sfx, rough=True):
    """The shared StageInputs of a case (computed once per session)."""
    return _cached(O, Nx, Ny, form, sfx, rough)
