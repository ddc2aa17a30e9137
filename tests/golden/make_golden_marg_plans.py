"""Records tests/golden/marg_plans.npz: the plans of the marginalisation packer for the cases of tests/marg_plan_cases.py, each packed
stand-alone and next to its solve problem (host only, no device):

    python tests/golden/make_golden_marg_plans.py [path of the library that packs]

The fixture was recorded from the packer as it stood before it was cut into phases (one function, pack_marg in tcv_marg.hip); record it again
only when a plan is MEANT to change, and say so in the commit."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
for p in (os.path.join(ROOT, "tc-viml_amd"), os.path.join(ROOT, "tests"), HERE):
    sys.path.insert(0, p)
if len(sys.argv) > 1:
    os.environ["TCV_LIB"] = os.path.abspath(sys.argv[1])
import tcv
import marg_plan_cases as mpc


def main():
    out = {}
    for name, (build, env) in mpc.cases(tcv).items():
        for mode in ("alone", "solve"):
            rec = mpc.record(tcv, build, env, mode == "solve")
            for k, v in rec.items():
                out["%s__%s__%s" % (name, mode, k)] = v
            if rec["rc"][0]:
                print("%-26s %-5s rc %d: %s" % (name, mode, rec["rc"][0], rec["err"].tobytes().decode()))
            elif rec["ints"].size == 0:
                print("%-26s %-5s keeps nothing" % (name, mode))
            else:
                H = mpc.header(tcv, rec["ints"])
                print("%-26s %-5s ints %5d doubles %5d  m %2d n %2d block_mode %d chunks %d cb_off %5d td_blk %2d disjoint %d prior_n %2d prior_abs %5d imu_abs %5d sqrt_src %2d"
                      % (name, mode, rec["ints"].size, rec["dlen"][0], H.m, H.n, H.block_mode, H.n_pchunk, H.cb_off, H.td_blk, H.proj_disjoint, H.prior_n,
                         H.prior_abs, H.imu_abs, H.sqrt_src))
    path = os.path.join(HERE, "marg_plans.npz")
    np.savez_compressed(path, **out)
    print("wrote marg_plans.npz: %d entries, %d bytes" % (len(out), os.path.getsize(path)))


if __name__ == "__main__":
    main()
