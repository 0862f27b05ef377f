"""CPU tier: the exact-weight attention probes of tests/test_encoder_lengths_gpu.py (tests/encoder_probes.py) have the properties its
assertions rely on, at every head width and length that file uses: the fp64 softmax formula on the probe inputs equals the closed-form
expectation to 1e-9, and in the one-hot / two-hot probes the weight outside the target keys is at most 1e-9 for every sequence and query —
a condition the inputs must meet, so that "one unit in the last place" on the GPU is a statement about the kernel."""
import numpy as np
import pytest

from tests import encoder_probes as ep

CASES = [(64, 160), (64, 288), (32, 160), (32, 288)]


@pytest.mark.parametrize("HD,L", CASES)
@pytest.mark.parametrize("kind", ep.PROBES)
def test_closed_form_is_the_fp64_softmax_and_nothing_leaks(kind, HD, L):
    qkv, lens, want = ep.build(kind, HD, L)
    assert qkv.shape == (L * L, 3 * ep.HEADS * HD) and qkv.dtype == np.float32 and lens.tolist() == list(range(1, L + 1))
    t1, t2 = (None, None) if kind == "uniform" else ep.targets(kind, L)
    out, leak = ep.softmax_f64(qkv, lens, HD, t1, t2)
    err = float(np.abs(out - want).max())                      # every query row, the ones behind the length included (their targets are live keys too)
    print(f"{kind} HD={HD} L={L}: closed form vs fp64 softmax {err:.3e}, largest weight off the targets {float(leak.max()):.3e}")
    assert err <= 1e-9
    assert ep.LEAK == 1e-9 and float(leak.max()) <= ep.LEAK
    if kind == "two-hot":                                      # the case leak_slack is there for: targets that cancel, closed form exactly 0
        assert (want[np.arange(L)[:, None] >= np.arange(L)[None, :]] == 0).any()
        vmax = float(np.abs(qkv.reshape(L, L, 3, ep.HEADS, HD)[:, :, 2]).max())
        assert err <= ep.leak_slack(kind, vmax) and ep.leak_slack("uniform", vmax) == 0.0
    assert not np.array_equal(want[:, :, 0], want[:, :, 1]) or kind == "uniform"          # head 1 is another draw than head 0
    x = qkv.reshape(L, L, 3, ep.HEADS, HD)
    assert not np.array_equal(x[:, :, 1, 0], x[:, :, 1, 1])


@pytest.mark.parametrize("HD,L", CASES)
def test_every_entry_is_exact_in_both_16_bit_types(HD, L):
    for kind in ep.PROBES:
        qkv, _, want = ep.build(kind, HD, L, vdtype="bf16")
        assert np.array_equal(ep.bf16_round(qkv), qkv) and np.array_equal(ep.f16_round(qkv), qkv)
        x = qkv.reshape(L, L, 3, ep.HEADS, HD)
        assert set(np.unique(x[:, :, 0])) <= {-16.0, 0.0, 16.0} and set(np.unique(x[:, :, 1])) == {-1.0, 1.0}
        if kind == "uniform":
            assert set(np.unique(x[:, :, 2])) == {0.0, 1.0}
        else:
            wide, _, _ = ep.build(kind, HD, L, vdtype="f16")
            assert np.array_equal(ep.f16_round(wide), wide) and not np.array_equal(ep.bf16_round(wide), wide)      # 11 significant bits
            assert 1.4 < float(x[:, :, 2].std()) < 1.6
        assert np.isfinite(want).all()


@pytest.mark.parametrize("L", [160, 288])
def test_targets_reach_the_first_and_the_last_live_key_and_every_chunk(L):
    lens = ep.lengths(L)
    t1, none = ep.targets("one-hot", L)
    assert (none == -1).all() and (t1 >= 0).all() and (t1 < lens[:, None]).all()
    for s in range(L):                                            # the queries that are compared: q < len
        n = int(lens[s])
        if n % 37:                                                # 37 is prime: the live queries' targets are a permutation of the live keys —
            assert sorted(t1[s, :n].tolist()) == list(range(n)), s      # the first, the last, every chunk and every position inside it
    assert all(n % 37 for n in (1, 2, 63, 64, 65, 127, 128, 129, 160, 255, 256, 257, 288))      # the lengths at a chunk or block edge are among them
    a, b = ep.targets("two-hot", L)
    h = (lens.astype(np.int64) + 1) // 2
    assert (a < h[:, None]).all() and ((b == -1) | ((b == a + h[:, None]) & (b < lens[:, None]))).all()
    assert (b[1:, :] >= 0).mean() > 0.9                           # nearly every query has its second maximum
    far = (b // 64 > a // 64)
    assert far[L - 1].all() and far[130:].mean() > 0.9            # ... in a later chunk than the first, for the longer sequences


def test_unit_in_the_last_place_of_both_types():
    assert ep.ulp16(1.0, "bfloat16") == 2.0 ** -7 and ep.ulp16(1.0, "float16") == 2.0 ** -10
    assert ep.ulp16(1.99, "bfloat16") == 2.0 ** -7 and ep.ulp16(2.0, "float16") == 2.0 ** -9 and ep.ulp16(-0.75, "float16") == 2.0 ** -11
    assert ep.ulp16(0.0, "float16") == 2.0 ** -24 and ep.ulp16(3e-6, "float16") == 2.0 ** -24 and ep.ulp16(2.0 ** -14, "float16") == 2.0 ** -24
    assert ep.ulp16(0.0, "bfloat16") == 2.0 ** -133
    x = np.float32([0.1, 3.3, 1e-3, 700.0])
    for name, rnd in (("bfloat16", ep.bf16_round), ("float16", ep.f16_round)):
        r = rnd(x).astype(np.float64)
        assert (np.abs(r - x) <= ep.ulp16(x, name) / 2).all() and (r != x).any()
    assert ep.bf16_round(np.float32([1.0 + 2.0 ** -8]))[0] == 1.0 and ep.bf16_round(np.float32([1.0 + 3 * 2.0 ** -8]))[0] == np.float32(1.0 + 2.0 ** -6)      # ties to even
