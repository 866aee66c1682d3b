"""Prepared verification keys, CPU tier: the window-width rule and the
run-length rule of csrc/prepared.hpp as pure functions (through the test
library, no GPU), the byte formula behind zk_vk_dev_bytes, and the exports."""
import ctypes as C

import pytest

PER_ENTRY = 96                     # a device affine G1 point
FIXED_WORDS = 144 + 2 * 48 * 68 + 4   # pairing.hpp: VK_IC, 32-bit words ahead of ic_g1


def plan(zkp, sound, num_public, force=0):
    v = [C.c_uint32(), C.c_uint32(), C.c_uint64(), C.c_uint64(), C.c_uint64()]
    rc = zkp.test_lib().zk_test_prepared_plan(C.c_int(int(sound)), C.c_uint64(num_public), C.c_int(force),
                                              *[C.byref(x) for x in v])
    assert rc == zkp.ZK_OK
    return tuple(x.value for x in v)   # width, windows, table bytes, device bytes, bound


def run_len(zkp, m, num_public, windows):
    run, fill = C.c_uint64(), C.c_uint64()
    rc = zkp.test_lib().zk_test_prepared_run(C.c_uint64(m), C.c_uint64(num_public), C.c_uint32(windows),
                                             C.byref(run), C.byref(fill))
    assert rc == zkp.ZK_OK
    return run.value, fill.value


def test_symbols_are_exported(zkp):
    lib = C.CDLL(zkp.LIB_PATH)
    for name in ("zk_vk_prepare", "zk_vk_dev_free", "zk_vk_dev_bytes", "zk_vk_dev_is_sound",
                 "zk_groth16_prepare_inputs", "zk_groth16_verify_many_prepared",
                 "zk_groth16_verify_many_bytes_prepared"):
        assert hasattr(lib, name), name
        assert name in zkp.EXPORTS
    t = zkp.test_lib()
    for name in ("zk_test_prepared_plan", "zk_test_prepared_run", "zk_test_prepared_force", "zk_test_prepared_info"):
        assert hasattr(t, name) and not hasattr(lib, name), name
    # no GPU is needed to refuse missing arguments
    assert lib.zk_vk_prepare(None, None, 0, None) == zkp.ZK_ERR_ARG
    assert lib.zk_vk_dev_bytes(None, None) == zkp.ZK_ERR_ARG
    assert lib.zk_groth16_prepare_inputs(None, None, None, 0, 0, None, None) == zkp.ZK_ERR_ARG
    assert lib.zk_groth16_verify_many_prepared(None, None, None, None, 0, 0, None) == zkp.ZK_ERR_ARG
    assert hasattr(zkp.VerificationKey, "prepare") and hasattr(zkp, "PreparedVerificationKey")


@pytest.mark.parametrize("sound", [False, True])
def test_width_rule(zkp, sound):
    bits = 255 if sound else 64
    bound = plan(zkp, sound, 1)[4]
    assert bound == 512 << 20
    last = 8
    for npub in (0, 1, 2, 3, 64, 256, 685, 686, 1000, 4096, 5825, 5826, 14563, 14564, 21931, 21932, 10 ** 6, 10 ** 9):
        b, W, table, dev, _ = plan(zkp, sound, npub)
        assert b in (0, 1, 2, 4, 8) and b <= last       # never wider for a longer key
        last = b
        if b == 0:                                      # nothing fits: not even b = 1
            assert npub * bits * PER_ENTRY > bound
            continue
        assert W == -(-bits // b)
        assert table == npub * W * ((1 << b) - 1) * PER_ENTRY <= bound
        assert dev == 4 * (FIXED_WORDS + 24 * (npub + 1)) + table
        if b < 8:                                       # the next wider table would not have fitted
            assert npub * -(-bits // (2 * b)) * ((1 << (2 * b)) - 1) * PER_ENTRY > bound
    # the issue's figures at b = 8, and the documented thresholds of a sound key
    assert plan(zkp, True, 1)[:3] == (8, 32, 783360)
    assert plan(zkp, False, 1)[:3] == (8, 8, 8 * 255 * 96)
    assert [plan(zkp, True, n)[0] for n in (1, 256, 685, 686, 4096, 5825, 5826)] == [8, 8, 8, 4, 4, 4, 2]
    assert [plan(zkp, False, n)[0] for n in (1, 256, 2741, 2742, 4096)] == [8, 8, 8, 4, 4]


def test_forced_width_reports_its_own_figures(zkp):
    for b, W in ((8, 32), (4, 64), (2, 128), (1, 255)):
        got = plan(zkp, True, 3, b)
        assert got[:3] == (b, W, 3 * W * ((1 << b) - 1) * PER_ENTRY)
    v = [C.c_uint32(), C.c_uint32(), C.c_uint64(), C.c_uint64(), C.c_uint64()]
    assert zkp.test_lib().zk_test_prepared_plan(1, C.c_uint64(3), 3, *[C.byref(x) for x in v]) == zkp.ZK_ERR_ARG


@pytest.mark.parametrize("npub,W", [(0, 32), (1, 8), (1, 32), (3, 32), (64, 32), (256, 32), (4096, 64), (130, 255)])
def test_run_length_rule(zkp, npub, W):
    T = npub * W
    _, fill = run_len(zkp, 1, npub, W)
    assert fill == 65536
    last = 0
    for m in (1, 2, 63, 64, 65, 130, 1000, 4096, 16384, 65535, 65536, 65537, 1 << 20):
        L, _ = run_len(zkp, m, npub, W)
        assert 1 <= L <= max(T, 1)
        assert L >= last                                 # longer runs for larger chunks, never shorter
        last = L
        if T <= 1:
            assert L == 1
            continue
        R = -(-T // L)
        if m >= fill:
            assert L == T                                # the whole proof in one lane
        else:
            root = next(s for s in range(1, T + 1) if s * s >= T)
            assert L >= root                             # a first-level lane never adds fewer than sqrt(T) ...
            if m * root <= fill:
                assert L == root and R <= root           # ... exactly that, and a second level as short, at small n
            else:
                assert m * R <= fill + m                 # else the first level stays near one wave per SIMD
    # more inputs never shorten the runs
    assert all(run_len(zkp, m, npub + 1, W)[0] >= run_len(zkp, m, npub, W)[0] for m in (1, 64, 4096, 65536))
