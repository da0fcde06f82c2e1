"""CPU tests of the anchor form of the fused RK3 stages (swmhd.h SWMHD_RK3_ANCHOR): the ABI refuses what it does not implement
before any HIP call, and the anchor variants of the row-marching kernels fit the register and LDS budgets of their siblings
(checked on a gfx950 cross-compile of the fast tendency object)."""
import ctypes
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL, ENOTSUP = 1, 3


def test_anchor_refusals_without_gpu(swmhd):
    B = swmhd._lib
    L = B.lib()
    bufs = [(ctypes.c_double * 256)() for _ in range(4)]     # (never dereferenced: every call below is refused first)
    ptr = [ctypes.cast(b, ctypes.c_void_p).value for b in bufs]
    p = ptr[0]
    arr = lambda k=0: B.ptr_array([ptr[k]] * 4)
    f = L.swmhd_tendencies_rk3_f64
    # q, qnew (must not alias q), Gn, Gm
    args = lambda Gm: (arr(0), arr(1), arr(2), Gm, 8, 8, 3, 3, 14, 1.0, 1.0, 9.81, 1.0, 1, 1, 0.1, 8.0 / 15.0, 0.25, 0, 0, 8)
    assert f(*args(None), B.RK3_ANCHOR | B.STRICT, None) == ENOTSUP
    assert f(*args(None), B.RK3_ANCHOR | B.BOUNDED_X, None) == ENOTSUP
    assert f(*args(arr(3)), B.RK3_ANCHOR | B.BOUNDED_Y, None) == ENOTSUP
    assert f(*args(arr(3)), B.RK3_ANCHOR | B.STRICT, None) == ENOTSUP
    assert f(*args(B.ptr_array([p, p, None, p])), B.RK3_ANCHOR, None) == EINVAL              # null W operand
    assert f(arr(0), arr(1), B.ptr_array([p, None, p, p]), None, *args(None)[4:], B.RK3_ANCHOR, None) == EINVAL   # null W output
    assert f(*args(arr(3)), B.RK3_ANCHOR | B.GM_IS_PREV_STATE, None) == EINVAL                # one operand form at a time
    t = L.swmhd_tendencies_f64                                                                  # no fused substep: nothing to anchor
    assert t(*([p] * 8), 8, 8, 3, 3, 14, 1.0, 1.0, 9.81, 1.0, 1, 1, 0, 8, B.RK3_ANCHOR, None) == EINVAL
    assert L.swmhd_step_rk3_f64(arr(0), arr(1), arr(2), arr(3), 8, 8, 3, 3, 14, 1.0, 1.0, 9.81, 1.0, 1, 1, 0.1, 1, B.BOUNDED_X, None, None) == ENOTSUP


HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
# the flags swmhd_amd/csrc/Makefile compiles tendency_fast.o with
FAST_FLAGS = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-ffp-contract=fast", "-fassociative-math", "-fno-signed-zeros",
              "-fno-trapping-math"]


def _resource_usage(tmp_path):
    out = subprocess.run([HIPCC, *FAST_FLAGS, "--offload-device-only", "-Rpass-analysis=kernel-resource-usage", "-c",
                          os.path.join(ROOT, "swmhd_amd", "csrc", "tendency_fast.hip"), "-o", str(tmp_path / "t.o")],
                         capture_output=True, text=True)
    assert out.returncode == 0, out.stderr[-2000:]
    res = {}
    for block in re.split(r"remark: [^\n]*Function Name: ", out.stderr)[1:]:
        name = block.split("\n")[0].split(" ")[0]
        num = lambda key: int(re.search(key + r": (\d+)", block).group(1))
        res[name] = dict(vgpr=num(r"VGPRs"), scratch=num(r"ScratchSize \[bytes/lane\]"), lds=num(r"LDS Size \[bytes/block\]"))
    return res


def _variants(res, kernel, mode):
    """{(template prefix without the mode): usage} of `kernel` instantiated with MODE `mode` (the last template argument)."""
    out = {}
    for name, u in res.items():
        m = re.search(kernel + r"I(.*)ELi" + str(mode) + r"EEEvNS_", name)
        if m:
            out[m.group(1)] = u
    return out


def test_anchor_variants_fit_the_budgets(tmp_path):
    """Anchor variants (MODE 9: first stage, MODE 11: later stages): no scratch in the vector-invariant and packed-fp32 kernels, the fp64
    vector-invariant ones within 168 VGPRs (3 workgroups of 256 per CU); the conservative fp64 ones, built for 3 workgroups per CU like
    the classic variants the step used (tendency_march_kernels.inc: CONS_W3_MODES), spill no more than those (MODE 5, 7); LDS equal to
    that of the classic variants everywhere."""
    res = _resource_usage(tmp_path)
    for kernel in ("k_tendency_vi_march", "k_tendency_cons_march", "k_tendency_vi_march_pk"):
        for mode, classic in ((9, 1), (11, 3)):
            new, old = _variants(res, kernel, mode), _variants(res, kernel, classic)
            assert new and set(new) == set(old), (kernel, mode)
            for key, u in new.items():
                assert u["lds"] == old[key]["lds"], (kernel, key, mode, u)
                if kernel == "k_tendency_cons_march" and key.startswith("d"):
                    spill = max(_variants(res, kernel, m)[key]["scratch"] for m in (5, 7))
                    assert u["scratch"] <= spill, (kernel, key, mode, u)
                else:
                    assert u["scratch"] == 0, (kernel, key, mode, u)
                if kernel == "k_tendency_vi_march" and key.startswith("d"):
                    assert u["vgpr"] <= 168, (kernel, key, mode, u)
