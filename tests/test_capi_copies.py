"""CPU checks of the grouped-window additions to the C boundary: the new entry
points are exported by the library they belong to, and the Python constant
matches include/zkp.h.  No compute calls (no GPU here)."""
import ctypes
import os
import re

HERE = os.path.dirname(os.path.abspath(__file__))
HEADER = os.path.join(HERE, "..", "include", "zkp.h")


def test_library_exports_the_copies_entry_points(zkp):
    lib = ctypes.CDLL(zkp.LIB_PATH)
    for name in ("zk_msm_g1_upload_copies", "zk_msm_g2_upload_copies", "zk_pk_device_bytes"):
        assert hasattr(lib, name), name
        assert name in zkp.EXPORTS


def test_test_library_exports_the_plan_hook(zkp):
    assert hasattr(zkp.test_lib(), "zk_test_pk_plan")
    assert "zk_test_pk_plan" in zkp.TEST_EXPORTS
    assert not hasattr(ctypes.CDLL(zkp.LIB_PATH), "zk_test_pk_plan")


def test_sound_copies_constant(zkp):
    assert zkp.ZK_OPT_SOUND_COPIES == 10
    m = re.search(r"ZK_OPT_SOUND_COPIES\s*=\s*(\d+)", open(HEADER).read())
    assert m and int(m.group(1)) == 10


def test_device_bytes_rejects_null(zkp):
    b = ctypes.c_uint64()
    assert zkp.lib().zk_pk_device_bytes(None, ctypes.byref(b)) == zkp.ZK_ERR_ARG
