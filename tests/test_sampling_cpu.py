"""CPU checks of the sampled decoder head: the numpy reference the GPU tests hold the kernel to, the new
C-ABI symbols, and the host-side argument checks of Engine.add_item."""
import numpy as np
import pytest

import sampling_ref as ref


@pytest.mark.parametrize("ctr,key,want", [
    ((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
    ((0xffffffff,) * 4, (0xffffffff,) * 2, (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
    ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0),
     (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1)),
])
def test_philox_known_answers(ctr, key, want):
    got = ref.philox4x32_10(*ctr, *key)
    assert tuple(int(x) for x in got) == want


def test_philox_vectorises_like_scalar_calls():
    c0 = np.arange(37, dtype=np.int64) * 977
    many = ref.philox4x32_10(c0, 5, 0, 0, 0x1234, 0xabcd)
    for i in (0, 1, 17, 36):
        one = ref.philox4x32_10(int(c0[i]), 5, 0, 0, 0x1234, 0xabcd)
        assert [int(m[i]) for m in many] == [int(o) for o in one]


def test_gumbel_noise_is_finite_and_keyed_on_seed_position_and_index():
    g = ref.gumbel(7, 3, 4099)
    assert g.dtype == np.float32 and np.isfinite(g).all()
    assert abs(float(g.mean()) - 0.5772) < 0.05           # Euler-Mascheroni: the Gumbel mean
    assert not np.array_equal(g, ref.gumbel(8, 3, 4099))
    assert not np.array_equal(g, ref.gumbel(7, 4, 4099))
    assert np.array_equal(g[:1000], ref.gumbel(7, 3, 1000))  # entry v does not depend on V


def _logits(seed, V):
    return np.random.default_rng(seed).standard_normal(V).astype(np.float32) * 3


@pytest.mark.parametrize("seed", range(5))
def test_k1_or_tiny_p_gives_the_argmax(seed):
    x = _logits(seed, 1000)
    am = ref.greedy(x)
    for s in range(8):
        assert ref.sample_row(x, 1.3, 1, 1.0, s, 5)[0] == am
        assert ref.sample_row(x, 0.7, 0, 1e-9, s, 5)[0] == am
        assert ref.sample_row(x, 0.7, 0, -0.5, s, 5)[0] == am  # P <= 0 keeps only the largest value


def test_temperature_to_zero_tends_to_greedy_and_zero_is_greedy():
    x = _logits(11, 500)
    am = ref.greedy(x)
    assert all(ref.sample_row(x, 1e-4, 0, 1.0, s, 9)[0] == am for s in range(16))
    for T in (0.0, -1.0, float("nan")):   # T == 0, and the device's out-of-domain T, decode greedily
        assert ref.sample_row(x, T, 3, 0.5, 1, 9)[0] == am


def test_kept_set_ties_nan_and_inf():
    x = np.array([1.0, 5.0, np.nan, 3.0, 5.0, -np.inf, 3.0, np.inf, 2.0], np.float32)
    keep, _ = ref.kept_set(x, 1.0, 3, 1.0)    # the 3rd largest finite value is 3.0: both 3.0 entries stay
    assert keep.tolist() == [False, True, False, True, True, False, True, False, False]
    keep, _ = ref.kept_set(x, 1.0, 0, 1.0)
    assert keep.tolist() == np.isfinite(x).tolist()
    keep, _ = ref.kept_set(x, 1.0, -4, 2.0)   # K < 0 acts as 0, P > 1 as 1
    assert keep.tolist() == np.isfinite(x).tolist()
    keep, _ = ref.kept_set(x, 1.0, 0, 0.5)    # 2 x e^5 against 2 x e^3 + e^2 + e^1: the two fives hold > 0.5
    assert keep.tolist() == [False, True, False, False, True, False, False, False, False]
    assert ref.sample_row(np.array([np.nan, -np.inf], np.float32), 1.0, 0, 1.0, 3, 4)[0] == -1
    assert ref.sample_row(x, 1.0, 0, 1.0, 3, 0)[0] == -1   # empty row


def test_draws_follow_the_softmax_of_the_kept_set():
    from scipy import stats
    x = np.array([2.0, 1.0, 0.5, 0.0, -1.0, 1.5], np.float32)
    T = 0.8
    toks = np.array([ref.sample_row(x, T, 0, 1.0, s, 3)[0] for s in range(6000)])
    q = np.exp(x / T - (x / T).max())
    q /= q.sum()
    obs = np.bincount(toks, minlength=len(x))
    assert stats.chisquare(obs, q * len(toks)).pvalue > 1e-3


def test_new_symbols_are_exported_and_scratch_sizes(mli):
    for n in ("mli_sample_scratch_bytes", "mli_sample_tokens", "mli_decoder_sampled_scratch_bytes",
              "mli_decoder_sampled", "mli_paged_decoder_sampled", "mli_engine_add_item_sampled"):
        assert hasattr(mli, n), n
    assert mli.mli_sample_scratch_bytes(1024, 1024) == 0
    assert mli.mli_sample_scratch_bytes(256, 50257) == 0
    assert mli.mli_decoder_sampled_scratch_bytes(1024, 1024) == 1024 * 1024 * 4   # the fp32 logits
    assert mli.mli_decoder_sampled_scratch_bytes(3, 65) == 3 * 65 * 4
    assert mli.mli_decoder_sampled_scratch_bytes(0, 65) == 0
    assert mli.mli_abi_version() == 4


def test_engine_add_item_rejects_bad_sampling_arguments_before_any_device_work():
    """Engine.add_item validates in Python before it reaches the library, so no engine (and no GPU) is needed here."""
    from min_llm_inference_amd.engine import sampling_params
    assert sampling_params(0.0, 0, 1.0, 0) is None              # the defaults: the plain entry point
    assert sampling_params(0.8, 0, 0.95, 5) == (0.8, 0, 0.95, 5)
    assert sampling_params(0.0, 0, 1.0, 9) == (0.0, 0, 1.0, 9)  # a seed alone still takes the sampled entry
    for bad in [(-0.1, 0, 1.0, 0), (float("nan"), 0, 1.0, 0), (float("inf"), 0, 1.0, 0), (1.0, -1, 1.0, 0),
                (1.0, 0, 0.0, 0), (1.0, 0, 1.5, 0), (1.0, 0, float("nan"), 0), (1.0, 0, 1.0, -1), (1.0, 0, 1.0, 2 ** 64)]:
        with pytest.raises(ValueError):
            sampling_params(*bad)
