"""Reference-mode setup, prove and sharding on general R1CS circuits
(tests/circuits.py), bit for bit against the CPU oracle's or_setup / or_prove
with the same parameters, r and s.  The synthetic x * y = z circuit of the
other tests has one unit entry per row, every variable named once and no
identity base out of step; these circuits have rows of 0, 1..3 and 40 entries
with values, repeated and out-of-range columns, a column as long as the
circuit, variables no row names or whose column cancels, several public inputs
and padded domains -- at 1000 x 777, 300 x 2500 and 4097 x 3000 (constraints x
variables; domains 1024, 512, 8192), the smallest that put several blocks of
every kernel to work.  tests/test_circuits_host.py pins those cases."""
import ctypes as C

import numpy as np
import pytest

import circuits as CZ
import gpu_util as U
import srs_util
from test_gpu_setup_size import SLOTS, _is_identity, _ref_rows, check_extras
from test_gpu_sound_copies import _pairing_accepts

pytestmark = pytest.mark.gpu

R = CZ.R
SEED = 0x6E0
IDS = ["%dx%d_pub%d" % s for s in CZ.SHAPES]
SMALL, MID, LARGE = CZ.SHAPES[1], CZ.SHAPES[0], CZ.SHAPES[2]     # domains 512, 1024, 8192


class Case:
    """one circuit with the oracle's key and proof for it"""

    def __init__(self, zkp, oracle, pyref, shape, unit_b=False):
        nc, V, num_public = shape
        self.circ = CZ.general_circuit(nc, V, num_public, SEED + nc, unit_b)
        self.num_public = num_public
        self.qap = zkp.QAP(zkp.CSRMatrices(nc, V, self.circ.mats))
        self.csr_o = oracle.CSR(nc, V, self.circ.mats)
        rng = pyref.SplitMix64(SEED + 7 * nc)
        self.params = [rng.fr() for _ in range(5)]
        self.r, self.s = rng.fr(), rng.fr()
        self.z = self.circ.z
        self._keys = {}
        self.oracle = oracle
        self.opk, self.ovk = self.okey(num_public)
        rc, self.oproof = oracle.prove(self.opk, self.csr_o, self.z, num_public, self.r, self.s)
        assert rc == 0

    def okey(self, num_public):
        if num_public not in self._keys:
            rc, opk, ovk = self.oracle.setup(self.csr_o, self.params, num_public,
                                             nthreads=self.oracle.default_threads())
            assert rc == 0
            self._keys[num_public] = (opk, ovk)
        return self._keys[num_public]


@pytest.fixture(scope="module", params=CZ.SHAPES, ids=IDS)
def case(request, zkp, oracle, pyref):
    return Case(zkp, oracle, pyref, request.param)


@pytest.fixture(scope="module")
def mid(zkp, oracle, pyref):
    return Case(zkp, oracle, pyref, MID)


def _device(z_rows):
    import torch
    return torch.from_numpy(np.ascontiguousarray(z_rows).view(np.int64).copy()).cuda()


def _make_key(zkp, ctx, cs, source, shard=0, nshards=1):
    """the two ways to a device key: the oracle's key uploaded, and the GPU setup straight into HBM"""
    if source == "uploaded":
        return U.pk_from_oracle(zkp, cs.opk, cs.qap, cs.num_public).upload(ctx, shard=shard, nshards=nshards)
    return zkp.CRS.generate_device(ctx, cs.qap, zkp.SetupParams(*cs.params), cs.num_public, shard=shard,
                                   nshards=nshards)


@pytest.fixture(scope="module")
def keys(ctx, zkp, case):
    ks = {src: _make_key(zkp, ctx, case, src) for src in ("uploaded", "made")}
    yield ks
    for k in ks.values():
        k.free()


@pytest.fixture(scope="module")
def mid_keys(ctx, zkp, mid):
    ks = {src: _make_key(zkp, ctx, mid, src) for src in ("uploaded", "made")}
    yield ks
    for k in ks.values():
        k.free()


# ------------------------------------------------------------------- setup ---
def _same_as_oracle(crs, opk, ovk):
    for nm in ("a_g1", "b_g1", "b_g2", "h_g1"):
        assert np.array_equal(getattr(crs.pk, nm), getattr(opk, nm)), nm
    assert np.array_equal(crs.pk.ic_g1, opk.ic_g1[:len(crs.pk.ic_g1)]), "ic_g1"
    for nm in ("alpha_g1", "beta_g1", "delta_g1", "beta_g2", "delta_g2"):
        assert np.array_equal(crs.pk.point(nm), opk.field(nm)), nm
    assert np.array_equal(crs.vk.ic_g1, ovk.ic_g1), "vk ic_g1"
    for nm in ("alpha_g1", "beta_g2", "gamma_g2", "delta_g2"):
        assert np.array_equal(crs.vk.point(nm), ovk.field(nm)), nm


def test_setup_equals_oracle(ctx, zkp, case):
    """csr_to_csc + k_colsum over columns of 0 to ~nc / 2 entries with values,
    k_setup_scalars' public / private split at 0, the shape's own and V - 1
    public inputs, and the host key's identity entries."""
    V = case.circ.V
    for num_public in sorted({0, case.num_public, V - 1}):
        opk, ovk = case.okey(num_public)
        crs = zkp.CRS.generate_from_qap(ctx, case.qap, zkp.SetupParams(*case.params), num_public)
        assert len(crs.pk.ic_g1) == V - num_public - 1 and len(crs.vk.ic_g1) == num_public + 1
        _same_as_oracle(crs, opk, ovk)


def test_setup_mixed_unit_matrices(ctx, zkp, oracle, pyref):
    """B without values (unit), A and C with them"""
    cs = Case(zkp, oracle, pyref, SMALL, unit_b=True)
    assert cs.qap.csr.s.b_val is None and cs.qap.csr.s.a_val and cs.qap.csr.s.c_val
    crs = zkp.CRS.generate_from_qap(ctx, cs.qap, zkp.SetupParams(*cs.params), cs.num_public)
    _same_as_oracle(crs, cs.opk, cs.ovk)
    # and the same matrices through the prover's row sums
    dpk = crs.pk.upload(ctx)
    try:
        proof = zkp.Prover.prove(dpk, zkp.Witness(cs.z, cs.num_public), r=cs.r, s=cs.s)
    finally:
        dpk.free()
    assert np.array_equal(proof.words, cs.oproof)


# -------------------------------------------------------------- device key ---
def _kept(cs, slot, shard, nshards):
    """the variables (H: coefficients) whose oracle base is not the identity
    and falls to this shard: all of them, or with 3 shards (no distributed
    quotient: contiguous ranges, strided H) the shard's range / stride"""
    num_public = cs.num_public
    ref = getattr(cs.opk, dict(SLOTS)[slot])
    if slot == 3:
        ref = ref[:cs.circ.V - num_public - 1]
    pos = np.arange(len(ref))
    if slot == 4:
        mine = pos % nshards == shard
    else:
        mine = (pos >= len(ref) * shard // nshards) & (pos < len(ref) * (shard + 1) // nshards)
    return pos[mine & ~_is_identity(ref)] + (num_public + 1 if slot == 3 else 0)


@pytest.mark.parametrize("shard,nshards", [(0, 1), (1, 3)])
@pytest.mark.parametrize("source", ["uploaded", "made"])
def test_device_key_holds_the_oracles_bases(ctx, zkp, oracle, case, source, shard, nshards):
    """The compacted slots of a device key: exactly the oracle's non-identity
    bases, in ascending variable order -- an irregular kept set in every slot."""
    dpk = _make_key(zkp, ctx, case, source, shard, nshards)
    try:
        assert dpk.test_info()[2:] == (shard, nshards)
        for slot, nm in SLOTS:
            idx, words, nex = dpk.test_bases(slot)
            want = _kept(case, slot, shard, nshards)
            assert np.array_equal(idx.astype(np.int64), want), (nm, len(idx), len(want))
            assert np.array_equal(words[:len(idx)], _ref_rows(case.opk, slot, idx, case.num_public)), nm
            assert nex == (0 if shard or slot in (3, 4) else (5 if slot in (0, 1) else 1)), nm
            if nex:
                check_extras(oracle, case.opk, slot, words, len(idx), nex)
        if nshards == 1:   # the kept sets are irregular: bases are missing in the middle of a slot
            for slot in (0, 1, 2, 3):
                want = _kept(case, slot, 0, 1)
                assert 0 < len(want) < want[-1] - want[0] + 1, slot
    finally:
        dpk.free()


# ------------------------------------------------------------------- prove ---
def _prove_both_ways(zkp, dpk, cs, dz):
    host = zkp.Prover.prove(dpk, zkp.Witness(cs.z, cs.num_public), r=cs.r, s=cs.s)
    dev = zkp.Prover.prove_device(dpk, dz.data_ptr(), len(cs.z), cs.num_public, cs.r, cs.s)
    return host, dev


@pytest.mark.parametrize("source", ["uploaded", "made"])
def test_prove_equals_oracle(zkp, case, keys, source):
    host, dev = _prove_both_ways(zkp, keys[source], case, _device(case.z))
    assert np.array_equal(host.words, case.oproof), "host witness"
    assert np.array_equal(dev.words, case.oproof), "device witness"


OPTIONS = [("schedule", 0), ("schedule", 3), ("schedule", -1), ("quotient_path", 1), ("quotient_path", 0),
           ("prove_win_c", 22)]


@pytest.mark.parametrize("option,value", OPTIONS, ids=["%s=%d" % o for o in OPTIONS])
def test_prove_under_every_path(ctx, zkp, mid, mid_keys, option, value):
    """The stream schedules, both quotient paths and the three-window plan on
    the 1024 domain: the oracle's proof every time, from both keys and both
    witness sources."""
    dz = _device(mid.z)
    made_here = {}
    try:
        if option == "schedule":
            ctx.set_schedule(value)
        elif option == "quotient_path":
            ctx.set_option(zkp.ZK_OPT_QUOTIENT_PATH, value)
        else:
            ctx.set_option(zkp.ZK_OPT_PROVE_WIN_C, value)     # governs keys made afterwards
            for src in ("uploaded", "made"):
                made_here[src] = _make_key(zkp, ctx, mid, src)
                assert made_here[src].test_info()[:2] == (3, 22)
        for src in ("uploaded", "made"):
            host, dev = _prove_both_ways(zkp, (made_here or mid_keys)[src], mid, dz)
            assert np.array_equal(host.words, mid.oproof), (src, "host witness")
            assert np.array_equal(dev.words, mid.oproof), (src, "device witness")
    finally:
        ctx.set_schedule(-1)
        ctx.set_option(zkp.ZK_OPT_QUOTIENT_PATH, -1)
        ctx.set_option(zkp.ZK_OPT_PROVE_WIN_C, 0)
        for k in made_here.values():
            k.free()


# ------------------------------------------------------- base-range shards ---
@pytest.mark.parametrize("nshards", [2, 3])
def test_sharded_prove_equals_oracle(ctx, zkp, case, nshards):
    """prove_partial per shard (each computing the whole quotient), then combine"""
    dz = _device(case.z)
    for source in ("uploaded", "made"):
        parts = []
        for k in range(nshards):
            dpk = _make_key(zkp, ctx, case, source, k, nshards)
            try:
                parts.append(zkp.Prover.prove_partial(dpk, dz.data_ptr(), len(case.z), case.num_public, case.r, case.s))
            finally:
                dpk.free()
        assert np.array_equal(zkp.Prover.combine(parts, case.r, case.s).words, case.oproof), source


# --------------------------------------------------- distributed quotient ---
@pytest.fixture(scope="module", params=[MID, LARGE], ids=[IDS[0], IDS[2]])
def dcase(request, zkp, oracle, pyref):
    return Case(zkp, oracle, pyref, request.param)


def _shard_keys(zkp, ctx, cs, source, N):
    return [_make_key(zkp, ctx, cs, source, k, N) for k in range(N)]


@pytest.mark.parametrize("source", ["uploaded", "made"])
@pytest.mark.parametrize("N", [2, 4, 8])
def test_distributed_quotient_equals_oracle(ctx, zkp, dcase, N, source):
    """N virtual ranks: stage A's row sums over each rank's rows, bases by
    variable owner, strided H -- on a circuit whose variables are named from
    rows of several ranks, of none, or only through a dropped column."""
    assert dcase.circ.domain % (N * N) == 0
    dz = _device(dcase.z)
    dpks = _shard_keys(zkp, ctx, dcase, source, N)
    try:
        proof = zkp.Prover.prove_virtual_shards(dpks, dz.data_ptr(), len(dcase.z), dcase.num_public, dcase.r, dcase.s)
    finally:
        for d in dpks:
            d.free()
    assert np.array_equal(proof.words, dcase.oproof)


class _NoExchange:
    """an attached exchange that is never used: the witness ranges are read, nothing is proved"""

    def all_to_all(self, send, recv, chunk):
        raise AssertionError("no transfer expected")

    def all_reduce_max(self, value):
        raise AssertionError("no agreement expected")

    def abort(self):
        pass


@pytest.mark.parametrize("N", [2, 4, 8])
def test_witness_ranges_follow_the_owners(zkp, case, N):
    """zk_groth16_witness_ranges of every rank against var_owner and
    pk_witness_ranges restated in tests/circuits.py: the rank's own variables
    (a variable no row names falls to rank v N / V, not to rank 0), z_0 and the
    columns of its rows; together the ranks read all of z, so a non-canonical
    entry anywhere is some rank's to reject."""
    circ = case.circ
    seen = np.zeros(circ.V, dtype=bool)
    with zkp.Context(0) as c:
        try:
            for k in range(N):
                c.attach_exchange(_NoExchange(), k, N)
                want = np.array(CZ.witness_ranges(circ, k, N), dtype=np.uint64)
                for source in ("uploaded", "made"):
                    dpk = _make_key(zkp, c, case, source, k, N)
                    try:
                        got = dpk.witness_ranges()
                    finally:
                        dpk.free()
                    assert np.array_equal(got, want), (k, source)
                for lo, hi in want:
                    seen[int(lo):int(hi)] = True
                own = [lo <= circ.unreferenced < hi for lo, hi in want]
                assert any(own) == (k == circ.unreferenced * N // circ.V)
        finally:
            c.detach_exchange()
    assert seen.all()


def test_non_canonical_entry_no_row_names(ctx, zkp, mid, mid_keys):
    """A valid witness whose entry at the variable no row names is r + 5: no
    row sum, base or public input reads it, and still the proof is refused --
    with the one-GPU prove's error on virtual ranks and on the host-witness
    path."""
    N = 4
    zb = mid.z.copy()
    zb[mid.circ.unreferenced] = CZ.fr_rows([R + 5])[0]
    dz = _device(zb)
    with pytest.raises(Exception) as single:
        zkp.Prover.prove_device(mid_keys["uploaded"], dz.data_ptr(), len(zb), mid.num_public, mid.r, mid.s)
    assert single.type is ValueError
    out = zkp._Proof()
    rc = zkp.lib().zk_groth16_prove(C.c_void_p(ctx._h), C.c_void_p(mid_keys["uploaded"]._h), zkp._p(zb),
                                    C.c_size_t(len(zb)), C.c_size_t(mid.num_public), C.byref(zkp._fr(mid.r)),
                                    C.byref(zkp._fr(mid.s)), C.byref(out))
    assert rc == zkp.ZK_ERR_ARG
    dpks = _shard_keys(zkp, ctx, mid, "uploaded", N)
    try:
        with pytest.raises(Exception) as virtual:
            zkp.Prover.prove_virtual_shards(dpks, dz.data_ptr(), len(zb), mid.num_public, mid.r, mid.s)
        assert virtual.type is single.type
        # any canonical value there: the oracle's proof, nothing reads the entry
        zc = mid.z.copy()
        zc[mid.circ.unreferenced] = CZ.fr_rows([R - 1])[0]
        dzc = _device(zc)
        proof = zkp.Prover.prove_virtual_shards(dpks, dzc.data_ptr(), len(zc), mid.num_public, mid.r, mid.s)
        assert np.array_equal(proof.words, mid.oproof)
    finally:
        for d in dpks:
            d.free()


# ---------------------------------------------------------------- verdicts ---
def test_verdicts_agree_with_the_oracle(ctx, zkp, oracle, case, keys):
    """One wrong variable breaks several rows at once: with row 1 among them
    the witness is invalid, without it the division fails (the last row nc - 1
    is among those), z_0 = 2 is invalid -- whatever or_prove says for the same
    witness, on one GPU (device and host witness) and on 4 virtual ranks."""
    circ = case.circ
    errors = {oracle.OR_ERR_INVALID_WITNESS: zkp.InvalidWitness, oracle.OR_ERR_QAP_DIVISION: zkp.PolynomialDivisionFailed}
    dpk = keys["uploaded"]
    dpks = _shard_keys(zkp, ctx, case, "uploaded", 4)
    try:
        seen = []
        for var, value in ((circ.shared_row1, (circ.z_int[circ.shared_row1] + 1) % R),
                           (circ.shared_last, (circ.z_int[circ.shared_last] + 1) % R), (0, 2)):
            zb = CZ.fr_rows(circ.witness_with(var, value))
            rc, _ = oracle.prove(case.opk, case.csr_o, zb, case.num_public, case.r, case.s)
            assert rc in errors, (var, rc)
            seen.append(rc)
            dz = _device(zb)
            with pytest.raises(errors[rc]):
                zkp.Prover.prove_device(dpk, dz.data_ptr(), len(zb), case.num_public, case.r, case.s)
            with pytest.raises(errors[rc]):
                zkp.Prover.prove_virtual_shards(dpks, dz.data_ptr(), len(zb), case.num_public, case.r, case.s)
            with pytest.raises(errors[rc]):   # z_0 != 1: the Witness constructor's own check (core:89-93)
                zkp.Prover.prove(dpk, zkp.Witness(zb, case.num_public), r=case.r, s=case.s)
        assert len(set(seen)) == 2            # both verdicts occurred
        # the good witness still proves afterwards, on both paths
        dz = _device(case.z)
        got = zkp.Prover.prove_device(dpk, dz.data_ptr(), len(case.z), case.num_public, case.r, case.s)
        assert np.array_equal(got.words, case.oproof)
        got = zkp.Prover.prove_virtual_shards(dpks, dz.data_ptr(), len(case.z), case.num_public, case.r, case.s)
        assert np.array_equal(got.words, case.oproof)
    finally:
        for d in dpks:
            d.free()


# ------------------------------------------------------------- evaluate_at ---
def test_evaluate_at_equals_pyref(ctx, zkp, oracle, pyref):
    """QAP.evaluate_at on the 512 domain against pyref.QAP.evaluate_at, at a
    random point and at the domain point w^5 (row 5: the cancelling pair)."""
    cs_nc, V, num_public = SMALL
    circ = CZ.general_circuit(cs_nc, V, num_public, SEED + cs_nc)
    qap = zkp.QAP(zkp.CSRMatrices(cs_nc, V, circ.mats))
    ref = CZ.pyref_qap(circ)
    w = pyref.root_of_unity(circ.domain)
    assert w == oracle.fr_root_of_unity(9)
    for t in (pyref.SplitMix64(SEED + 3).fr(), pow(w, 5, R)):
        ev = qap.evaluate_at(t, circ.z, ctx)
        assert [ev.a_val, ev.b_val, ev.c_val] == ref.evaluate_at(t, circ.z_int)
        assert ev.z_val == (pow(t, circ.domain, R) - 1) % R
    assert ref.evaluate_at(pow(w, 5, R), circ.z_int) == circ.row_values(5)


# -------------------------------------------------------------- sound mode ---
def test_sound_prove_is_accepted(ctx, zkp, pyref, mid):
    """A sound key made on the device for the general circuit: the proof
    passes the pairing check with the true public inputs and fails it with one
    of them changed."""
    circ, num_public = mid.circ, mid.num_public
    vk = zkp.VerificationKey(num_public, sound=True)
    dpk = zkp.CRS.generate_device(ctx, mid.qap, zkp.SetupParams(*mid.params), num_public, sound=True, vk=vk)
    try:
        assert dpk.sound
        proof = zkp.Prover.prove(dpk, zkp.Witness(mid.z, num_public), r=mid.r, s=mid.s)
        dz = _device(mid.z)
        assert zkp.Prover.prove_device(dpk, dz.data_ptr(), len(mid.z), num_public, mid.r, mid.s) == proof
    finally:
        dpk.free()
    x = circ.z_int[1:num_public + 1]
    assert len(x) == 3
    assert _pairing_accepts(zkp, ctx, pyref, vk, proof, x)
    assert zkp.Verifier.verify(vk, proof, x) is True
    for k in range(num_public):
        bad = list(x)
        bad[k] = (bad[k] + 1) % R
        assert not _pairing_accepts(zkp, ctx, pyref, vk, proof, bad), k
        assert zkp.Verifier.verify(vk, proof, bad) is False


def test_sound_key_from_a_string(ctx, zkp, pyref, mid):
    """CRS.from_srs on a string of the circuit's domain size: the sound setup's
    key for (alpha, beta, 1, 1, tau), entry for entry."""
    rng = pyref.SplitMix64(SEED + 4)
    par = {"alpha": rng.fr(), "beta": rng.fr(), "tau": rng.fr()}
    assert mid.circ.domain == 1 << 10
    srs = srs_util.string(zkp, ctx, par, 10)
    crs = zkp.CRS.from_srs(ctx, mid.qap, srs, mid.num_public)
    want = srs_util.trusted(zkp, ctx, mid.qap, par, mid.num_public)
    srs_util.same_crs(crs, want)
    ident = [0] * 12 + [1]
    for v in (mid.circ.unreferenced, mid.circ.cancelling):
        assert list(crs.pk.a_g1[v]) == ident
    assert list(crs.pk.a_g1[mid.circ.duplicate]) != ident
