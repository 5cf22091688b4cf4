"""Which test holds kernel X to a reference, as a committed fact ("Kernel coverage record").

tests/kernel_coverage.json records, for every device kernel of the library, the test files whose gpu-marked tests launch it: one
rocprofv3 --kernel-trace pass per file on the MI355X (tools/kernel_coverage.py collect / merge, outside pytest).  This file holds,
without a GPU:
  - the inventory of the build (tools/kernel_inventory.py on min_llm_inference_amd/build) equals the record's key set: a kernel
    the record does not name fails with its name (a new hipLaunchKernelGGL instantiation, a new template argument), and so does a
    stale entry;
  - every kernel is launched by at least one file of JUDGED_FILES -- the files that compare a kernel's numeric output, element by
    element, with the float64 model or the CPU oracle.  Engine, replay, dispatch, scratch-contract and bit-identity-only files
    tie kernels to each other or to tokens and do not qualify;
  - EXEMPT names only kernels that produce no floating-point result a model could judge, and only kernels that still exist;
  - the name normalisation maps a symbol-table name and a profiler name of one kernel to one key;
  - the check itself fails on a record with one key deleted and on one with a kernel's only judged file deleted.
To refresh the record after adding a kernel: add the case that launches it to the judged file of its family, then on the MI355X
`python tools/kernel_coverage.py collect --files <the files that changed>` and `python tools/kernel_coverage.py merge`."""
import copy
import json
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import kernel_coverage as kc  # noqa: E402
import kernel_inventory as ki  # noqa: E402

BUILD = os.path.join(ROOT, "min_llm_inference_amd", "build")
BUILD_COMMAND = 'python -c "import __graft_entry__ as g; g.build()"'
RECORD = os.path.join(ROOT, "tests", "kernel_coverage.json")
HEADS_FILE = "tests/test_heads_instantiations_gpu.py"

# file -> what it compares element by element, and with what
JUDGED_FILES = {
    "tests/test_naive_kernels_gpu.py": "contiguous kernels and their composition, whole tensors against the CPU oracle",
    "tests/test_paged_kernels_gpu.py": "paged kernels, GEMMs and compositions, whole tensors and the whole pool against the CPU oracle",
    "tests/test_paged_bf16_gpu.py": "bf16 paged kernels against the CPU oracle on the rounded inputs",
    "tests/test_paged_fp8_gpu.py": "fp8 paged kernels against the CPU oracle on what the pages hold",
    "tests/test_lean_path_gpu.py": "the lean scans and compositions against the CPU oracle",
    "tests/test_encoder_decoder_gpu.py": "encoder and greedy decoder head, whole tensors and the whole pool against the CPU oracle",
    "tests/test_golden_gpu.py": "the decode step against committed vectors of the CPU oracle",
    "tests/test_drawn_shapes_gpu.py": "kernels and compositions at drawn shapes against the CPU oracle",
    "tests/test_full_size_properties_gpu.py": "the benchmark shapes against the CPU oracle on whole rows",
    "tests/test_attention_accuracy_gpu.py": "every attention entry point against the float64 model",
    "tests/test_stream_partition_gpu.py": "the equal-shares scan against the float64 model on adversarial length vectors",
    "tests/test_heads_scan_gpu.py": "the multi-head scan against the per-head float64 model",
    "tests/test_window_scan_gpu.py": "the windowed scans against the windowed float64 model",
    "tests/test_sinks_scan_gpu.py": "the scans with sink tokens against the sink-windowed float64 model",
    "tests/test_gqa_scan_gpu.py": "the grouped-query scan against the float64 model on the expanded operands",
    "tests/test_alibi_scan_gpu.py": "the ALiBi scan against the float64 model with the bias",
    "tests/test_softcap_scan_gpu.py": "the capped scan against the float64 model with the cap",
    "tests/test_sink_logits_scan_gpu.py": "the sink-logit scan against the float64 model with the sink",
    HEADS_FILE: "every multi-head decode instantiation against its family's float64 model",
    "tests/test_prompt_scan_gpu.py": "the prompt scan against the float64 model on the virtual rows",
    "tests/test_prompt_long_gpu.py": "the prompt scans at n_sequence 4096 against the float64 model",
    "tests/test_softcap_prompt_gpu.py": "the capped prompt scan and its scoring against the float64 model",
    "tests/test_sink_logits_prompt_gpu.py": "the sink-logit prompt scan and its scoring against the float64 model",
    "tests/test_prompt_score_gpu.py": "the scoring of given tokens against the float64 log-probability model",
    "tests/test_logprobs_gpu.py": "the log-probability heads against the float64 log-probability model",
    "tests/test_sampling_gpu.py": "the sampled decoder head, token by token against the float64 numpy reference of its contract",
    "tests/test_gemm_edges_gpu.py": "projection, prefill and logits GEMMs, every written value against the float64 GEMM model",
    "tests/test_rope_gemm_gpu.py": "the rotary projection and fills, the whole pool against the float64 judge",
    "tests/test_rope_scan_gpu.py": "the rotary lean composition against the float64 attention model on the rotated state",
    "tests/test_shape_limits_gpu.py": "every launcher at its last accepted shape against the float64 models",
}
# kernel -> why no model can judge it (no floating-point result of its own) and which test checks it bit-exactly
EXEMPT = {
    "mli::stream_copy_kernel(HIP_vector_type<float, 4u>const*, HIP_vector_type<float, 4u>*, unsigned long)":
        "a copy: tests/test_lean_path_gpu.py::test_stream_copy_copies_every_bit compares every bit",
}
NEVER_EXEMPT = ("scan", "gemm", "sample", "softmax", "qkt", "encoder", "decoder")


def unjudged(record, judged=JUDGED_FILES, exempt=EXEMPT):
    """the kernels of the record that no judged file launches and no exemption names"""
    return sorted(k for k, files in record.items() if k not in exempt and not set(files) & set(judged))


def mismatch(inventory, record):
    """(kernels of the build the record does not name, entries of the record the build does not have)"""
    return sorted(set(inventory) - set(record)), sorted(set(record) - set(inventory))


@pytest.fixture(scope="module")
def inventory():
    if not os.path.isdir(BUILD) or not any(n.endswith(".o") for n in os.listdir(BUILD)):
        pytest.fail(f"no build at {os.path.relpath(BUILD, ROOT)}: run {BUILD_COMMAND}")
    names = ki.inventory(BUILD)
    assert len(names) > 400, "the unbundling found only part of the library"
    return names


@pytest.fixture(scope="module")
def record():
    with open(RECORD) as f:
        return json.load(f)


def test_the_inventory_equals_the_record(inventory, record):
    missing, stale = mismatch(inventory, record)
    assert not missing, (f"{len(missing)} kernels of the build have no entry in tests/kernel_coverage.json -- add a judged case that "
                         "launches each and re-take the record (tools/kernel_coverage.py):\n" + "\n".join(missing))
    assert not stale, f"{len(stale)} entries of tests/kernel_coverage.json name no kernel of the build:\n" + "\n".join(stale)


def test_the_record_is_names_only_and_sorted(record):
    assert list(record) == sorted(record)
    known = set(kc.gpu_test_files())
    for kernel, files in record.items():
        assert files and files == sorted(set(files)), kernel
        assert set(files) <= known, f"{kernel}: {sorted(set(files) - known)} are no test files with gpu-marked tests"


def test_every_kernel_is_judged(record):
    bare = unjudged(record)
    assert not bare, (f"{len(bare)} kernels are launched by no file of JUDGED_FILES -- add the smallest case that dispatches each to "
                      "the judged file of its family:\n" + "\n".join(f"{k}   <- {record[k]}" for k in bare))


def test_judged_files_are_gpu_test_files_with_a_reason():
    known = set(kc.gpu_test_files())
    for name, reason in JUDGED_FILES.items():
        assert name in known, f"{name} is no test file with gpu-marked tests"
        assert reason and "\n" not in reason
    for name in known:
        kind = os.path.basename(name)
        if any(word in kind for word in ("engine", "replay", "dispatch", "scratch", "resident")):
            assert name not in JUDGED_FILES, f"{name} ties kernels to each other or to tokens"


def test_exemptions_are_stated_and_small(inventory):
    assert len(EXEMPT) <= 8
    for kernel, reason in EXEMPT.items():
        assert reason and "\n" not in reason
        assert kernel in inventory, f"the exemption of {kernel} names no kernel of the build"
        for word in NEVER_EXEMPT:
            assert word not in kernel.lower(), f"{kernel}: a {word} kernel has a result a model can judge"


def test_every_multi_head_decode_instantiation_is_in_the_grid_file(record):
    """4 families x E 2 x NJ 2 x NT 2 x forms 3 x GQA 2 = 192, all launched by tests/test_heads_instantiations_gpu.py"""
    names = ("heads_decode_scan_kernel", "heads_alibi_scan_kernel", "heads_softcap_scan_kernel", "heads_sink_logits_scan_kernel")
    grid = [k for k in record if any(f"mli::{n}<" in k for n in names)]
    assert len(grid) == 192
    missing = [k for k in grid if HEADS_FILE not in record[k]]
    assert not missing, "\n".join(missing)


SYMBOL = ("_ZN3mli23heads_alibi_scan_kernelINS_8ElemBF16ELi2ELb1ELb1ELb1ELb1EEEvPKfPKPKvPKiPfP15HIP_vector_typeIfLj2EESA_iiiiiiiPjiiiS3_")
KEY = ("void mli::heads_alibi_scan_kernel<mli::ElemBF16, 2, true, true, true, true>(float const*, void const*const*, int const*, "
       "float*, HIP_vector_type<float, 2u>*, float*, int, int, int, int, int, int, int, unsigned int*, int, int, int, float const*)")


@pytest.mark.parametrize("name", [
    SYMBOL,                                        # the function symbol
    SYMBOL + ".kd",                                # its kernel descriptor
    KEY,                                           # the profiler's Kernel_Name
    KEY + ".kd",
    KEY + " [clone .kd]",                          # a demangler's note for the descriptor
    KEY.replace("const*const*", "const* const*").replace(", ", ","),
    '"' + KEY.replace("2u>*", "2u> *") + '"\n',    # a quoted CSV field
])
def test_one_key_per_kernel(name):
    assert ki.normalise(name) == KEY


def test_normalisation_keeps_instantiations_apart():
    a = "void mli::gemm_bf16_mfma_kernel<2, 1, 128, false>(mli::GemmArgs)"
    b = "void mli::gemm_bf16_mfma_kernel<2, 1, 128, true>(mli::GemmArgs)"
    assert ki.normalise(a) == a and ki.normalise(b) == b
    assert ki.normalise("mli::softmax_lengths_kernel(float*, int const*, int, int)") == "mli::softmax_lengths_kernel(float*, int const*, int, int)"
    assert ki.normalise("void f<mli::A<1> >(int)") == ki.normalise("void f<mli::A<1>>(int)")


def test_merge_keeps_the_library_kernels_under_their_keys():
    raw = {"tests/test_b_gpu.py": [KEY + ".kd", "void at::native::vectorized_elementwise_kernel<4, float>(int)"],
           "tests/test_a_gpu.py": [SYMBOL, "mli::softmax_lengths_kernel(float*, int const*, int, int)"]}
    assert kc.merge_names(raw) == {KEY: ["tests/test_a_gpu.py", "tests/test_b_gpu.py"],
                                   "mli::softmax_lengths_kernel(float*, int const*, int, int)": ["tests/test_a_gpu.py"]}


def test_a_deleted_key_fails_the_check(inventory, record):
    mutant = copy.deepcopy(record)
    gone = sorted(mutant)[len(mutant) // 2]
    del mutant[gone]
    assert mismatch(inventory, mutant) == ([gone], [])
    assert mismatch(inventory + ["void mli::new_kernel<1>(int)"], record)[0] == ["void mli::new_kernel<1>(int)"]


def test_a_deleted_judged_file_fails_the_check(record):
    single = [k for k, files in record.items() if k not in EXEMPT and len(set(files) & set(JUDGED_FILES)) == 1]
    assert single, "no kernel hangs on a single judged file"
    mutant = copy.deepcopy(record)
    (only,) = set(mutant[single[0]]) & set(JUDGED_FILES)
    mutant[single[0]].remove(only)
    assert unjudged(mutant) == [single[0]]
    assert single[0] in unjudged(record, judged={k: v for k, v in JUDGED_FILES.items() if k != only})


def test_time_limits_cover_every_gpu_file():
    for name in kc.gpu_test_files():
        assert os.path.basename(name) in kc.UNPROFILED_SECONDS, f"{name}: no duration in tools/kernel_coverage.py"
        assert kc.limit_for(name) >= kc.MIN_LIMIT
