"""The QAP chain in its linear form, H = zinv (icoset(a b) - ifft(c)) (csrc/ntt.hip ntt_qap_linear; tune
qap_linear, default 1): c takes one inverse transform instead of a coset round trip, the first pass of H's inverse
coset transform forms a b and its last pass subtracts c.  Every comparison is bit-exact.

* H coefficients (mi_groth16_h_coeffs_dev) against the oracle at d = 2^10 (one pass, unfused kernels), 2^11 (the
  smallest two-pass plan, 1 + 10 bits) and 2^13, under qap_linear x qap_fused in {0, 1}^2; at 2^11 also for a
  witness that does not satisfy the R1CS (the identity holds for every witness);
* d = 2^19 (the smallest three-pass plan, 5 + 4 + 10 bits): qap_linear = 1 equals qap_linear = 0 for a satisfying
  and an altered witness, and one proof passes the pairing check.
"""
import itertools

import numpy as np
import pytest

import circuits
import fil_groth16 as fg

pytestmark = pytest.mark.gpu

COMBOS = list(itertools.product((0, 1), (0, 1)))  # (qap_linear, qap_fused)


def _h_dev(ctx, gc, zb):
    import torch

    zd = torch.from_numpy(np.frombuffer(zb, dtype=np.uint8).copy()).cuda()
    hbuf = torch.zeros(32 * gc.d, dtype=torch.uint8, device="cuda")
    fg.h_coeffs_dev(ctx, gc, zd.data_ptr(), hbuf.data_ptr())
    return hbuf.cpu().numpy().tobytes()


def _altered(zb, n_vars):
    """the witness with its last aux value changed by one"""
    v = (int.from_bytes(zb[32 * (n_vars - 1):32 * n_vars], "little") + 1) % fg.FR_MODULUS
    return zb[:32 * (n_vars - 1)] + v.to_bytes(32, "little")


@pytest.mark.parametrize("log_d,rows,seed,unsat", [(10, 700, 101, False), (11, 1500, 102, False),
                                                   (11, 1500, 102, True), (13, 5000, 103, False)])
def test_h_coeffs_vs_oracle(ctx, oracle, tune, log_d, rows, seed, unsat):
    import split_oracle

    n_in, n_aux, rws, z = circuits.random_circuit(seed, rows, n_in=6, n_free=32)
    mats = circuits.to_csr(rws)
    oc = oracle.OracleCircuit(len(rws), n_in, n_aux, mats)
    gc = fg.Circuit(ctx, len(rws), n_in, n_aux, mats)
    assert gc.d == 1 << log_d
    zb = circuits.z_bytes(z)
    if unsat:
        zb = _altered(zb, n_in + n_aux)
    want = split_oracle.h_coeffs_perm(oracle.OracleParams(oc, circuits.toxic(seed)), zb)
    if not unsat:  # coefficient d - 1 (the last bit-reversed position) of a satisfying witness is exactly 0
        assert want[-32:] == bytes(32)
    for linear, fused in COMBOS:
        tune.set("qap_linear", linear)
        tune.set("qap_fused", fused)
        got = _h_dev(ctx, gc, zb)
        if unsat:  # the oracle drops coefficient d - 1, the device keeps it: compared between the chains below
            got = got[:-32] + bytes(32)
        assert got == want, (linear, fused)
    if unsat:
        tune.set("qap_fused", 1)
        tune.set("qap_linear", 0)
        old = _h_dev(ctx, gc, zb)
        assert old[-32:] != bytes(32)  # a b - c is not divisible by Z: the witness is indeed unsatisfying
        tune.set("qap_linear", 1)
        assert _h_dev(ctx, gc, zb) == old


def test_three_pass_plan(ctx, oracle, tune):
    import torch

    from fil_groth16 import synth

    sc = synth.SynthCircuit(19, 4, 5)
    gc = sc.load(ctx)
    assert gc.d == 1 << 19
    zb = sc.z_bytes()
    for w in (zb, _altered(zb, sc.num_vars)):
        tune.set("qap_linear", 0)
        old = _h_dev(ctx, gc, w)
        tune.set("qap_linear", 1)
        new = _h_dev(ctx, gc, w)
        assert new == old
        assert (new[-32:] == bytes(32)) == (w is zb)
    tune.clear("qap_linear")
    pk = fg.generate_random_parameters(ctx, gc, circuits.toxic())
    zd = torch.from_numpy(np.frombuffer(zb, dtype=np.uint8).copy()).cuda()
    r, s = circuits.blinding(3)
    raw = fg.prove(ctx, pk, gc, zd.data_ptr(), r, s, want_raw=True)[1]
    vk, ic = pk.verifying_key()
    assert oracle.groth16_verify(vk, ic, zb[:32 * sc.n_in], raw)
