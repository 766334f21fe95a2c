"""One rank of a sharded run that passes only ITS elements to the device-pointer entries, as bench.py --gpus N does, for
tests/test_gpu_device_entries.py (launched by torch.distributed.run with the gloo control plane; every rank drives GPU 0
through tests/fake_rccl).  Every rank makes the same calls in the same order: the host entries (which pick the rank's elements
themselves), stan_host_partition_elements, then stan_hip_assemble_hex8_dev on the picked elements and stan_hip_cg_solve_dev,
all arrays guarded (tests/device_buffers.py).  Checked here, bit for bit: info() with row_begin / row_end / n_halo / n_blocks,
U, iterations, termination type and residual; guards intact, inputs unchanged, every entry of d_U written on every rank."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402
import torch.distributed as dist  # noqa: E402
from stan_amd import hip, host, problem  # noqa: E402
from tests import device_buffers as B  # noqa: E402

spec, out_dir = sys.argv[1], sys.argv[2]
rank, world = int(os.environ["RANK"]), int(os.environ["WORLD_SIZE"])
dist.init_process_group("gloo")
if spec.startswith("fuzz:"):   # tests/fuzz.py job: shuffled wire order, several neighbours, empty ranks
    from tests import fuzz
    job = fuzz.random_job(int(spec[5:]))
else:
    job = problem.cube_job(int(spec), jitter=0.05)
ctx = hip.Context(0)
box = [ctx.unique_id() if rank == 0 else None]
dist.broadcast_object_list(box, 0)
ctx.comm_init(rank, world, box[0])

K = ctx.assemble_hex8(job.xyz, job.node_dof, job.conn, job.elem_mat, job.elem_type, job.mat_E_nu, job.red)
want_info = K.info()
U, rep = K.cg_solve(job.F, 1e-8)
K.free()

mine = host.partition_elements(job.node_index, job.conn, world, rank)
dev = "cuda:0"
mesh = B.Mesh(job, dev, offset=rank % 2, conn=job.conn[mine], elem_mat=job.elem_mat[mine], elem_type=job.elem_type[mine])
dF = B.input_("F", job.F, B.guard_len(job.n_dof), dev, rank % 2)
dU = B.output("U", job.n_red, B.guard_len(job.n_dof), dev, rank % 2)
torch.cuda.synchronize()
Kd = ctx.assemble_hex8_dev(*mesh.assemble_args())
got_info = Kd.info()
got = Kd.cg_solve_dev(dF.ptr, dU.ptr, 1e-8)
Kd.free()
torch.cuda.synchronize()

# (every assertion behind the last collective: a rank that stops early would leave its peers waiting in an exchange)
assert mine.shape[0] == want_info["n_elements_on_device"] and (np.diff(mine) > 0).all(), (mine.shape[0], want_info["n_elements_on_device"])
assert got_info == want_info, (got_info, want_info)
B.check(mesh.inputs + [dF, dU])
assert dU.numpy().tobytes() == U.tobytes(), "rank %d: U differs in %d entries" % (rank, int((dU.numpy() != U).sum()))
assert got == rep and np.float64(got["rel_residual"]).tobytes() == np.float64(rep["rel_residual"]).tobytes(), (got, rep)
print("rank %d: rows [%d, %d), %d of %d elements, halo %d: %s" %
      (rank, want_info["row_begin"], want_info["row_end"], mine.shape[0], job.conn.shape[0], want_info["n_halo"], rep), flush=True)
np.savez(os.path.join(out_dir, "rank%d.npz" % rank), U=dU.numpy(), its=rep["iterations"], term=rep["terminationtype"],
         n_picked=mine.shape[0], n_elem=job.conn.shape[0])
ctx.close()
dist.barrier()
dist.destroy_process_group()
