"""The measured figures of tests/test_gemm_rows_ksteps_gpu.py and tests/test_batch24_gpu.py, kept for one pytest run and written to the
path GEMM_ROWS_KSTEPS_ERRORS names (profiles/gemm_rows_ksteps_errors.txt is such a run on one MI355X)."""
import os

_LINES = {}              # section -> {key: line}

HEAD = ("Measured by tests/test_gemm_rows_ksteps_gpu.py and tests/test_batch24_gpu.py on one MI355X (written when GEMM_ROWS_KSTEPS_ERRORS\n"
        "names a path).\n"
        "rounding: standard-normal operands and bias through cn_gemm_rows_grouped_k; ratio = the largest |got - ref|_ij /\n"
        "(2 (K + S + 2) 2^-24 A_ij), A = the float64 product of |A| and |B| plus |bias|, S = 4 (the K quarters are combined once, after\n"
        "the last chunk); the test holds every ratio at <= 1.\n"
        "bank / generator: relative L2 error of each gradient against the float64 MLPs (the generator's from the cotangents that reached\n"
        "its five MLP outputs in the same run), with the AdaIN MLPs as one bank and layer by layer; the tests hold bank <= 4 x layerwise.\n")


def note(section, key, line):
    _LINES.setdefault(section, {})[key] = line
    path = os.environ.get("GEMM_ROWS_KSTEPS_ERRORS")
    if not path:
        return
    with open(path, "w") as f:
        f.write(HEAD)
        for sec in sorted(_LINES):
            f.write("\n[%s]\n" % sec)
            for k in sorted(_LINES[sec]):
                f.write(_LINES[sec][k] + "\n")
