"""GPU call matrix of the output-frame kernel (swmhd_output_fields_*, swmhd_ensemble_output_fields_*), through the C-ABI alone.

The yardstick is the numpy restatement tests/output_cases.np_output_fields (pinned on the CPU by tests/test_output_cases_cpu.py) applied
to output_cases.images(parents), what the WRAP flags make of the parents.  The object is built without FMA contraction and with IEEE
divide and sqrt, so EVERY comparison is bitwise (helpers.same_bits: NaN in the same places, the same integer bits elsewhere, so -0.0 is
not 0.0): float64 frames against the restatement, float32 frames against the restatement rounded to float32.

Layout of every call.  Parents: row stride Nx + 2 Hx + 5, member stride rows * sy + 11, NaN in every gap and in every halo cell that
output_cases.keep_mask does not name (so every halo cell of a wrapped direction); h = 1 + 0.3 rand.  Frame: a sentinel-filled buffer,
7 elements of lead, out_stride_y = Nx + 3, out_stride_f = rows * osy + 5, out_stride_m = nf * osf + 9.  After a call every element it
does not own still holds the sentinel and every parent is bitwise what it was."""
import functools

import numpy as np
import pytest
import torch

import output_cases as OC
from helpers import same_bits

pytestmark = pytest.mark.gpu
NP = {"f64": np.float64, "f32": np.float32}
TORCH = {"f64": torch.float64, "f32": torch.float32}
SENT = -777.25
DX, DY = 0.1, 0.12
WRAP_X, WRAP_Y = OC.WRAP_X, OC.WRAP_Y
WRAPS = (0, WRAP_X, WRAP_Y, WRAP_X | WRAP_Y)
ALL = OC.ALL


def _real(x, sfx):
    """a spacing as the kernel receives it (an f32 call passes floats through the C-ABI)"""
    return x if sfx == "f64" else float(np.float32(x))


def _sel(which):
    """the fields of a frame, slot by slot: slot f holds the f-th set bit of `which`"""
    return [k for k in range(len(OC.NAMES)) if which >> k & 1]


def _parents(Nx, Ny, Hx, Hy, sfx, seed, form, wrap=0):
    """Four random parents in the model type, NaN in every halo cell that no frame cell of this formulation reads under these flags."""
    rng = np.random.default_rng(seed)
    shape = (Ny + 2 * Hy, Nx + 2 * Hx)
    q = [rng.standard_normal(shape), rng.standard_normal(shape), 1.0 + 0.3 * rng.random(shape), rng.standard_normal(shape)]
    out = []
    for a, p in zip(q, OC.PARENTS):
        keep = OC.keep_mask(Nx, Ny, Hx, Hy, form, p, wrap)
        keep[Hy:Hy + Ny, Hx:Hx + Nx] = True
        out.append(np.where(keep, a, np.nan).astype(NP[sfx]))
    return out


class Device:
    """Parents on the device with a pitched row stride and a pitched member stride, NaN in every gap; `lead` elements before the base"""

    def __init__(self, members_parents, Nx, Ny, Hx, Hy, sfx, lead=0):
        self.Nx, self.Ny, self.Hx, self.Hy, self.sfx, self.lead = Nx, Ny, Hx, Hy, sfx, lead
        self.members = len(members_parents)
        Py, Px = Ny + 2 * Hy, Nx + 2 * Hx
        self.sy = Px + 5
        self.stride_m = Py * self.sy + 11
        self.host, self.t = [], []
        for k in range(4):
            host = np.full(lead + self.members * self.stride_m, np.nan, dtype=NP[sfx])
            for m, q in enumerate(members_parents):
                o = lead + m * self.stride_m
                host[o:o + Py * self.sy].reshape(Py, self.sy)[:, :Px] = q[k]
            self.host.append(host)
            self.t.append(torch.from_numpy(host).cuda())

    def ptrs(self, member=0):
        return [t.data_ptr() + (self.lead + member * self.stride_m) * t.element_size() for t in self.t]

    def assert_untouched(self):
        it = np.int64 if self.sfx == "f64" else np.int32
        for k, (t, host) in enumerate(zip(self.t, self.host)):
            assert np.array_equal(t.cpu().numpy().view(it), host.view(it)), f"parent {OC.PARENTS[k]} was written to"


@functools.lru_cache(maxsize=None)
def _owned(total, lead, members, nf, nrows, Nx, osm, osf, osy):
    idx = (lead + np.arange(members)[:, None, None, None] * osm + np.arange(nf)[None, :, None, None] * osf
           + np.arange(nrows)[None, None, :, None] * osy + np.arange(Nx)[None, None, None, :])
    own = np.zeros(total, dtype=bool)
    own[idx.ravel()] = True
    return idx, own


def _frame_call(S, dev, form, rows, which, out_sfx, flags, mode="single", member=0, lead=7, pad_y=3):
    """One call of swmhd_[ensemble_]output_fields_* into a sentinel-filled buffer with pitched row, field and member strides.
    Returns the fields (members, nf, nrows, Nx) -- (nf, nrows, Nx) for a single grid -- after checking every other element for the sentinel."""
    L = S._lib.lib()
    j0, j1 = rows
    nrows, nf, Nx = j1 - j0, bin(which).count("1"), dev.Nx
    osy = Nx + pad_y
    osf = nrows * osy + 5
    osm = nf * osf + 9
    members = dev.members if mode == "ensemble" else 1
    buf = torch.full((lead + members * osm + 7,), SENT, dtype=TORCH[out_sfx], device="cuda")
    optr = buf.data_ptr() + lead * buf.element_size()
    grid = (dev.Nx, dev.Ny, dev.Hx, dev.Hy, dev.sy, DX, DY, form)
    frame = (j0, j1, which, optr, buf.element_size(), osy, osf)
    stream = S.fields._stream_ptr()
    if mode == "single":
        rc = getattr(L, f"swmhd_output_fields_{dev.sfx}")(*dev.ptrs(member), *grid, *frame, flags, stream)
    else:
        rc = getattr(L, f"swmhd_ensemble_output_fields_{dev.sfx}")(*dev.ptrs(), members, dev.stride_m, *grid, *frame, osm, flags, stream)
    S._lib.check(rc, "swmhd_output_fields")
    flat = buf.cpu().numpy()
    idx, own = _owned(flat.size, lead, members, nf, nrows, Nx, osm, osf, osy)
    assert (flat[~own] == SENT).all(), f"sentinel overwritten: which={which} rows={rows} {mode} at {np.flatnonzero((flat != SENT) & ~own)[:8].tolist()}"
    got = flat[idx]
    return got[0] if mode == "single" else got


# --- 1. one grid: every shape, halo, formulation, precision, frame type, mask, row range and wrap ------------------------------------------
@pytest.mark.parametrize("sfx", ["f64", "f32"])
@pytest.mark.parametrize("Hx,Hy", OC.HALOS, ids=[f"halo{hx}{hy}" for hx, hy in OC.HALOS])
@pytest.mark.parametrize("Nx,Ny", OC.SHAPES, ids=[f"{nx}x{ny}" for nx, ny in OC.SHAPES])
def test_frames_match_the_restatement_bitwise(swmhd, Nx, Ny, Hx, Hy, sfx):
    S = swmhd
    dx, dy = _real(DX, sfx), _real(DY, sfx)
    for wrap in WRAPS:
        for form in (1, 0):
            q = _parents(Nx, Ny, Hx, Hy, sfx, 100 * Nx + Ny + wrap + form, form, wrap)
            ref = OC.images(q, Nx, Ny, Hx, Hy, wrap)
            dev = Device([q], Nx, Ny, Hx, Hy, sfx)
            want = OC.np_output_fields(*ref, Nx, Ny, Hx, Hy, dx, dy, form)
            assert np.isfinite(want).all(), "the restatement reached a NaN halo cell"
            for j0, j1 in OC.ROW_RANGES(Ny):
                part = OC.np_output_fields(*ref, Nx, Ny, Hx, Hy, dx, dy, form, rows=(j0, j1))
                assert np.array_equal(part, want[:, j0:j1])
                for which in OC.MASKS:
                    for out_sfx in ("f32", "f64"):
                        got = _frame_call(S, dev, form, (j0, j1), which, out_sfx, wrap)
                        same_bits(got, part[_sel(which)],
                                  f"{Nx}x{Ny} halo {Hx},{Hy} {sfx} form {form} wrap {wrap} rows {j0}:{j1} mask {which} -> {out_sfx}")
            dev.assert_untouched()


# --- 2. every mask ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sfx", ["f64", "f32"])
@pytest.mark.parametrize("form", [1, 0], ids=["vi", "cons"])
@pytest.mark.parametrize("Nx,Ny", [(5, 2), (1, 1)], ids=["5x2", "1x1"])
def test_every_mask_is_the_matching_rows_of_the_whole_frame(swmhd, Nx, Ny, form, sfx):
    """All 127 masks: a load condition that is wrong for one of them gives a number that is not the all-seven frame's."""
    S = swmhd
    dx, dy = _real(DX, sfx), _real(DY, sfx)
    for Hx, Hy in OC.HALOS:
        for wrap in (0, WRAP_X | WRAP_Y):
            q = _parents(Nx, Ny, Hx, Hy, sfx, 17 + Nx + wrap, form, wrap)
            dev = Device([q], Nx, Ny, Hx, Hy, sfx)
            whole = _frame_call(S, dev, form, (0, Ny), ALL, "f64", wrap)
            want = OC.np_output_fields(*OC.images(q, Nx, Ny, Hx, Hy, wrap), Nx, Ny, Hx, Hy, dx, dy, form)
            assert np.isfinite(want).all()
            same_bits(whole, want, f"{Nx}x{Ny} halo {Hx},{Hy} {sfx} form {form} wrap {wrap} all seven")
            for which in OC.ALL_MASKS:
                got = _frame_call(S, dev, form, (0, Ny), which, "f64", wrap)
                same_bits(got, whole[_sel(which)], f"{Nx}x{Ny} halo {Hx},{Hy} {sfx} form {form} wrap {wrap} mask {which}")
            dev.assert_untouched()


# --- 3. non-finite parent cells ---------------------------------------------------------------------------------------------------------------
NAN_CELLS = lambda Nx, Ny: ((0, (3, 4)), (WRAP_X | WRAP_Y, (0, 0)), (WRAP_X | WRAP_Y, (Ny - 1, Nx - 1)), (0, (Ny - 1, 0)))


@pytest.mark.parametrize("sfx", ["f64", "f32"])
def test_a_nan_in_one_cell_of_one_parent(swmhd, sfx):
    """One NaN in an interior cell of each parent in turn: the NaN set of every field is the restatement's, and field by field it is the
    set of cells that output_cases.FIELD_REACH says read that cell."""
    S = swmhd
    Nx, Ny, Hx, Hy = 7, 9, 3, 2
    dx, dy = _real(DX, sfx), _real(DY, sfx)
    for wrap, cell in NAN_CELLS(Nx, Ny):
        for k, p in enumerate(OC.PARENTS):
            for form in (1, 0):
                q = _parents(Nx, Ny, Hx, Hy, sfx, 77, form, wrap)
                q[k][Hy + cell[0], Hx + cell[1]] = np.nan
                dev = Device([q], Nx, Ny, Hx, Hy, sfx)
                want = OC.np_output_fields(*OC.images(q, Nx, Ny, Hx, Hy, wrap), Nx, Ny, Hx, Hy, dx, dy, form)
                reach = np.stack([OC.reached_cells(Nx, Ny, form, n, p, cell, wrap) for n in OC.NAMES])
                print("parent", p, "cell", cell, "wrap", wrap, "form", form, "NaN per field", reach.sum(axis=(1, 2)).tolist())
                assert reach.any() and np.array_equal(np.isnan(want), reach)
                for out_sfx in ("f64", "f32"):
                    got = _frame_call(S, dev, form, (0, Ny), ALL, out_sfx, wrap)
                    assert np.array_equal(np.isnan(got), reach), f"NaN in {p} at {cell}, wrap {wrap}, form {form}: not the cells of REACH"
                    same_bits(got, want, f"NaN in {p} at {cell}, wrap {wrap}, form {form} -> {out_sfx}")
                dev.assert_untouched()


@pytest.mark.parametrize("sfx", ["f64", "f32"])
def test_an_infinite_depth_gives_zeros_not_nan(swmhd, sfx):
    """One +Inf in h, conservative form: uh / Inf, vh / Inf and the B of the faces around are zeros (of the dividend's sign), the h frame
    holds the Inf, nothing is NaN; the bits of the restatement."""
    S = swmhd
    Nx, Ny, Hx, Hy = 7, 9, 3, 2
    dx, dy = _real(DX, sfx), _real(DY, sfx)
    for wrap, (J, I) in NAN_CELLS(Nx, Ny):
        q = _parents(Nx, Ny, Hx, Hy, sfx, 78, 0, wrap)
        q[2][Hy + J, Hx + I] = np.inf
        dev = Device([q], Nx, Ny, Hx, Hy, sfx)
        want = OC.np_output_fields(*OC.images(q, Nx, Ny, Hx, Hy, wrap), Nx, Ny, Hx, Hy, dx, dy, 0)
        assert not np.isnan(want).any() and np.isinf(want).sum() == 1 and want[2, J, I] == np.inf
        assert want[0, J, I] == 0 and want[1, J, I] == 0 and want[5, J, I] == 0 and want[6, J, I] == 0
        for out_sfx in ("f64", "f32"):
            same_bits(_frame_call(S, dev, 0, (0, Ny), ALL, out_sfx, wrap), want, f"+Inf in h at {(J, I)}, wrap {wrap} -> {out_sfx}")
        dev.assert_untouched()


# --- 4. the sign of zero ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sfx", ["f64", "f32"])
@pytest.mark.parametrize("form", [1, 0], ids=["vi", "cons"])
def test_signed_zeros_of_a_constant_A_at_rest(swmhd, form, sfx):
    """Constant A, u = v = 0: B_x = -((A - A) / dy) / h is -0.0 by the written order, B_y and s are +0.0, in every cell."""
    S = swmhd
    dx, dy = _real(DX, sfx), _real(DY, sfx)
    for Nx, Ny, Hx, Hy in ((5, 2, 3, 2), (7, 9, 1, 1)):
        for wrap in (0, WRAP_X | WRAP_Y):
            q = _parents(Nx, Ny, Hx, Hy, sfx, 3, form, wrap)
            for k, c in ((0, 0.0), (1, 0.0), (3, 0.75)):
                q[k][~np.isnan(q[k])] = c
            dev = Device([q], Nx, Ny, Hx, Hy, sfx)
            want = OC.np_output_fields(*OC.images(q, Nx, Ny, Hx, Hy, wrap), Nx, Ny, Hx, Hy, dx, dy, form)
            for out_sfx in ("f64", "f32"):
                got = _frame_call(S, dev, form, (0, Ny), ALL, out_sfx, wrap)
                tag = f"{Nx}x{Ny} {sfx} form {form} wrap {wrap} -> {out_sfx}"
                same_bits(got, want, tag)
                for f in (4, 5, 6):
                    assert (got[f] == 0).all(), tag
                assert np.signbit(got[5]).all(), tag + ": B_x is -0.0"
                assert not np.signbit(got[6]).any() and not np.signbit(got[4]).any(), tag + ": B_y and s are +0.0"
            dev.assert_untouched()


# --- 5. the ensemble entry point ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("members", [1, 3])
@pytest.mark.parametrize("sfx", ["f64", "f32"])
@pytest.mark.parametrize("Nx,Ny", [(5, 2), (65, 3)], ids=["5x2", "65x3"])
def test_ensemble_call_is_the_single_call_per_member(swmhd, Nx, Ny, sfx, members):
    """Pitched stride_m and out_stride_m, a sentinel in every gap: member m is bitwise the single-grid call on that member's parents (and
    the restatement); a member full of NaN leaves the others alone."""
    S = swmhd
    Hx, Hy = 3, 2
    dx, dy = _real(DX, sfx), _real(DY, sfx)
    for wrap in (0, WRAP_X | WRAP_Y):
        for form in (1, 0):
            qs = [_parents(Nx, Ny, Hx, Hy, sfx, 31 + m, form, wrap) for m in range(members)]
            dev = Device(qs, Nx, Ny, Hx, Hy, sfx)
            dirty = [[a.copy() for a in q] for q in qs]
            if members > 1:
                for a in dirty[1]:
                    a[:] = np.nan
            dev_dirty = Device(dirty, Nx, Ny, Hx, Hy, sfx)
            refs = [OC.images(q, Nx, Ny, Hx, Hy, wrap) for q in qs]
            for which in (ALL, OC.mask_of("u", "v", "A", "s"), OC.mask_of("s")):
                for rows in ((0, Ny), (1, Ny)):
                    for out_sfx in ("f64", "f32"):
                        tag = f"{Nx}x{Ny} {sfx} members {members} wrap {wrap} form {form} mask {which} rows {rows} -> {out_sfx}"
                        ens = _frame_call(S, dev, form, rows, which, out_sfx, wrap, mode="ensemble")
                        assert ens.shape == (members, len(_sel(which)), rows[1] - rows[0], Nx)
                        for m in range(members):
                            same_bits(ens[m], _frame_call(S, dev, form, rows, which, out_sfx, wrap, member=m), tag + f" member {m} vs single")
                            want = OC.np_output_fields(*refs[m], Nx, Ny, Hx, Hy, dx, dy, form, rows=rows)[_sel(which)]
                            assert np.isfinite(want).all()
                            same_bits(ens[m], want, tag + f" member {m} vs restatement")
                        if members > 1:
                            bad = _frame_call(S, dev_dirty, form, rows, which, out_sfx, wrap, mode="ensemble")
                            assert np.isnan(bad[1]).all()
                            same_bits(bad[0], ens[0], tag + " member 0 beside a NaN member")
                            same_bits(bad[2], ens[2], tag + " member 2 beside a NaN member")
                            assert not np.array_equal(ens[0], ens[2])
            dev.assert_untouched()
            dev_dirty.assert_untouched()


# --- 6. bases that are only element-aligned -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sfx,out_sfx", [("f64", "f32"), ("f32", "f64")])
def test_under_aligned_bases(swmhd, sfx, out_sfx):
    """The frame one element past an allocation with an odd out_stride_y, the parents one element past theirs: a layout the ABI documents
    as legal (only element alignment is promised), bitwise the call on bases at the allocations."""
    S = swmhd
    Nx, Ny, Hx, Hy = 65, 3, 3, 2
    dx, dy = _real(DX, sfx), _real(DY, sfx)
    for form in (1, 0):
        for wrap in (0, WRAP_X | WRAP_Y):
            q = _parents(Nx, Ny, Hx, Hy, sfx, 41, form, wrap)
            want = OC.np_output_fields(*OC.images(q, Nx, Ny, Hx, Hy, wrap), Nx, Ny, Hx, Hy, dx, dy, form)
            at_base, past = Device([q], Nx, Ny, Hx, Hy, sfx, lead=0), Device([q], Nx, Ny, Hx, Hy, sfx, lead=1)
            assert all(a % 256 == 0 for a in at_base.ptrs()) and all(a % 256 == past.t[0].element_size() for a in past.ptrs())
            for rows in ((0, Ny), (1, Ny)):
                aligned = _frame_call(S, at_base, form, rows, ALL, out_sfx, wrap, lead=0, pad_y=3)
                odd = _frame_call(S, past, form, rows, ALL, out_sfx, wrap, lead=1, pad_y=4)
                assert (Nx + 4) % 2 == 1
                tag = f"{sfx} -> {out_sfx} form {form} wrap {wrap} rows {rows}"
                same_bits(odd, aligned, tag + ": under-aligned vs aligned")
                same_bits(odd, want[:, rows[0]:rows[1]], tag + ": under-aligned vs restatement")
            at_base.assert_untouched()
            past.assert_untouched()
