"""Runs one named set of the CAP-form checks of tests/test_softcap_gpu.py in this process, under the
DLT_CE_* knobs its environment holds (the launcher reads them once per process):

    python -m tests.softcap_ref_child <set>

Prints each check's name, its VARIANT and RATIO lines; exits non-zero at the first check that fails."""
import os
import sys
import traceback


def main(argv):
    from tests import softcap_ref as S
    if len(argv) != 2 or argv[1] not in S.CAP_CHILD_SETS:
        print(f"usage: python -m tests.softcap_ref_child {{{','.join(S.CAP_CHILD_SETS)}}}")
        return 2
    knobs, keys = S.CAP_CHILD_SETS[argv[1]]
    wrong = {k: os.environ.get(k) for k, v in knobs.items() if os.environ.get(k) != v}
    if wrong:
        print(f"set {argv[1]} needs {knobs} in the environment, found {wrong}")
        return 2
    from tests import test_softcap_gpu as T
    print(f"set {argv[1]}: {len(keys)} checks, knobs {knobs}", flush=True)
    for key in keys:
        print(f"CHECK {key}", flush=True)
        try:
            T.check_cap(key)
        except BaseException:  # the first failure ends the run: nothing more is started on the GPU
            traceback.print_exc()
            print(f"FAILED {key}", flush=True)
            return 1
    print("ALL PASSED", flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv))
