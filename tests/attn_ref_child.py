"""Runs one named set of the checks of tests/test_attn_kernels_gpu.py in this process, under the
work schedule its environment selects (attention.hip reads DLT_ATTN_SCHED / DLT_ATTN_XCD once per
process), and saves every output of every case for the parent's bitwise comparison:

    python -m tests.attn_ref_child <set> <outputs.pt>

Prints each check's name and RATIO lines; exits non-zero at the first check that fails."""
import os
import sys
import traceback


def main(argv):
    from tests import attn_ref as R
    if len(argv) != 3 or argv[1] not in R.CHILD_SETS:
        print(f"usage: python -m tests.attn_ref_child {{{','.join(R.CHILD_SETS)}}} <outputs.pt>")
        return 2
    knobs, names = R.CHILD_SETS[argv[1]]
    mine = {k: os.environ.get(k) for k in ("DLT_ATTN_SCHED", "DLT_ATTN_XCD")}
    if any(mine[k] != knobs.get(k) for k in mine) or R.sched_of(os.environ) != R.sched_of(knobs):
        print(f"set {argv[1]} needs exactly {knobs} in the environment, found {mine}")
        return 2
    import torch
    from tests import test_attn_kernels_gpu as T
    print(f"set {argv[1]}: {len(names)} cases, schedule {T.SCHED}", flush=True)
    for name in names:
        print(f"CHECK {name}", flush=True)
        try:
            T.run_check(name)
        except BaseException:  # the first failure ends the run: nothing more is started on the GPU
            traceback.print_exc()
            print(f"FAILED {name}", flush=True)
            return 1
    torch.save({n: T.OUTPUTS[n] for n in names}, argv[2])
    print("ALL PASSED", flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv))
