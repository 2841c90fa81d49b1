"""worker of tests/test_gpu_shard_boundary.py::test_natural_workgroup_numbering_in_a_fresh_process: SBMBP_SHARD_XCD is read once
per process, so the test starts this script with the variable in its environment. One threshold case (tests/
shard_boundary_graph.py) with the ranks as threads, two damped sweeps queued in one call and three undamped ones in the next
(inside a call a sweep reads what the send pass of the sweep before shipped), the state and the reported difference after
either call written to the .npz named first. Arguments: out Q dc world n_chunks."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
for p in (ROOT, HERE):
    sys.path.insert(0, p)

import sbm_bp_amd as S  # noqa: E402
import shard_boundary_graph as sg  # noqa: E402


def main():
    out, Q, dc, world, n_chunks = sys.argv[1], int(sys.argv[2]), int(sys.argv[3]), int(sys.argv[4]), int(sys.argv[5])
    S.load_library()
    d, psi, msg, _ = sg.run_case(S, sg.instance(Q, dc, world), n_chunks)
    np.savez(out, d=d, psi=psi, msg=msg, xcd=os.environ.get("SBMBP_SHARD_XCD", ""))


if __name__ == "__main__":
    main()
