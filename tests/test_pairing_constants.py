"""CPU checks of the device pairing's constants: the committed constants.hpp
is what gen_constants.py prints, and the x-power chain of the final
exponentiation's hard part (csrc/pairing.hpp) is the multiple c of
(p^4 - p^2 + 1) / r the package documents (FINAL_EXP_C)."""
import contextlib
import io
import math
import os
import re
import runpy

P = 0x1A0111EA397FE69A4B1BA7B6434BACD764774B84F38512BF6730D2A0F6B0F6241EABFFFEB153FFFFB9FEFFFFFFFFAAAB
R = 0x73EDA753299D7D483339D80809A1D80553BDA402FFFE5BFEFFFFFFFF00000001
X = -0xD201000000010000


def test_generator_reproduces_committed_constants(zkp):
    buf = io.StringIO()
    with contextlib.redirect_stdout(buf):
        runpy.run_path(os.path.join(zkp.CSRC, "gen_constants.py"), run_name="__main__")
    with open(os.path.join(zkp.CSRC, "constants.hpp")) as f:
        assert f.read() == buf.getvalue()


def test_hard_part_chain_is_c_times_the_exponent(zkp):
    c = zkp.FINAL_EXP_C
    with open(os.path.join(zkp.CSRC, "pairing.hpp")) as f:
        assert re.search(r"PR_FINAL_EXP_C = (\d+);", f.read()).group(1) == str(c)
    assert c in (1, 3) and math.gcd(c, R) == 1
    assert (P ** 4 - P * P + 1) % R == 0
    # f12_final_exp: m^(x-1), ^(x-1), ^(x+p), ^(x^2+p^2-1), times m^3
    chain = (X - 1) ** 2 * (X + P) * (X * X + P * P - 1) + 3
    assert chain == c * ((P ** 4 - P * P + 1) // R)
    # with the easy part (p^6 - 1)(p^2 + 1) in front: c (p^12 - 1) / r
    assert (P ** 6 - 1) * (P * P + 1) * chain == c * ((P ** 12 - 1) // R)
