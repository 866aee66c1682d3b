"""CPU checks of the phase-2 contribution code (csrc/ceremony.hip): the scalar
split the endomorphism walk relies on, over pyref alone, with beta as
gen_constants.py emits it; the new entry points are declared and exported and
refuse a NULL context.  No GPU."""
import ctypes
import os
import re

import points_util as U

X_ABS = 0xD201000000010000          # x = -X_ABS
RQ_DEV = 392                        # device Montgomery: R = 2^392 (gen_constants.py)


def _beta(zkp):
    """ENDO_BETA32 of constants.hpp as a canonical integer"""
    with open(os.path.join(zkp.CSRC, "constants.hpp")) as f:
        m = re.search(r"\bENDO_BETA32\[12\] = \{(.*?)\};", f.read())
    words = [int(w, 16) for w in re.findall(r"0x[0-9a-f]{8}", m.group(1))]
    assert len(words) == 12
    return sum(w << (32 * i) for i, w in enumerate(words)) * pow(1 << RQ_DEV, -1, U.PMOD) % U.PMOD


def test_scalar_split(zkp, pyref):
    """k P = e1 P + (-e2) phi(P) with (e2, e1) = divmod(k, x^2), both halves
    below 2^128, for three scalars: a random one, r - 1, and x^2 + 1."""
    beta = _beta(zkp)
    assert beta == pow(2, (pyref.P - 1) // 3, pyref.P)
    x2 = X_ABS * X_ABS
    assert pyref.R == x2 * x2 - x2 + 1
    pt = U.g1_points(4)[2]
    phi = (pt[0] * beta, pt[1])
    assert pyref.G1.on_curve(phi)
    for k in (pyref.SplitMix64(0xC0171).fr(), pyref.R - 1, x2 + 1):
        e2, e1 = divmod(k, x2)
        assert e1 < 1 << 128 and e2 < 1 << 128
        want = pyref.G1.mul(pt, k)
        got = pyref.G1.add(pyref.G1.mul(pt, e1), pyref.G1.mul(pyref.G1.neg(phi), e2))
        assert got == want, hex(k)


def test_symbols(zkp):
    lib = ctypes.CDLL(zkp.LIB_PATH)
    for name in ("zk_g1_mul_scalar", "zk_groth16_contribute_sound", "zk_groth16_verify_contribution_sound"):
        assert hasattr(lib, name) and name in zkp.EXPORTS, name
    assert not hasattr(lib, "zk_test_g1_mul_scalar_plain")        # the plain walk is the test library's
    assert hasattr(zkp.test_lib(), "zk_test_g1_mul_scalar_plain")
    assert "zk_test_g1_mul_scalar_plain" in zkp.TEST_EXPORTS
    hdr = open(os.path.join(os.path.dirname(zkp.CSRC), "..", "include", "zkp.h")).read()
    for name in ("ZK_CONTRIB_OK = 0", "ZK_CONTRIB_SHAPE", "ZK_CONTRIB_FIXED_PART", "ZK_CONTRIB_POINT",
                 "ZK_CONTRIB_DELTA", "ZK_CONTRIB_RATIO"):
        assert name in hdr
    assert (zkp.ZK_CONTRIB_OK, zkp.ZK_CONTRIB_SHAPE, zkp.ZK_CONTRIB_FIXED_PART, zkp.ZK_CONTRIB_POINT,
            zkp.ZK_CONTRIB_DELTA, zkp.ZK_CONTRIB_RATIO) == tuple(range(6))


def test_null_context_is_refused(zkp):
    L = zkp.lib()
    k = zkp._fr(5)
    pts = (zkp._G1 * 1)()
    pk, vk = zkp._PK(), zkp._VK()
    st = ctypes.c_int(-1)
    assert L.zk_g1_mul_scalar(None, pts, ctypes.c_size_t(1), ctypes.byref(k), pts) == zkp.ZK_ERR_ARG
    assert L.zk_groth16_contribute_sound(None, ctypes.byref(pk), ctypes.byref(vk), ctypes.byref(k)) == zkp.ZK_ERR_ARG
    assert L.zk_groth16_verify_contribution_sound(None, ctypes.byref(pk), ctypes.byref(vk), ctypes.byref(pk),
                                                  ctypes.byref(vk), None, ctypes.c_size_t(0),
                                                  ctypes.byref(st)) == zkp.ZK_ERR_ARG
    assert zkp.test_lib().zk_test_g1_mul_scalar_plain(None, pts, ctypes.c_size_t(1), ctypes.byref(k),
                                                      pts) == zkp.ZK_ERR_ARG
