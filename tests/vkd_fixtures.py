"""The VKD jobs the CPU and GPU tests share (hekaton_system_amd/vkd_circuit.py), each built once per curve and never changed:
A = append, update, update of one user (`VkdJob.random(log_n = 5)`); B = append X, append Y, update X; both at depth 32,
split 4, N = 32.  `small` is depth 16, split 2, U = 2 (N = 16)."""
import functools

from hekaton_system_amd.vkd_circuit import Append, SparseTree, Update, VkdJob, concat, get_index

CHAL = (0x1234567, 0x89ABCDE)
DEPTH, SPLIT = 32, 4


@functools.lru_cache(maxsize=None)
def job_a(curve, chal=True):
    job = VkdJob.random(curve, 5, DEPTH, SPLIT)
    if chal:
        job.set_challenges(*CHAL)
    return job


def updates_b(curve, depth=DEPTH):
    """(initial root, final root, [append X, append Y, update X]) over a tree that holds the genesis user."""
    tree = SparseTree(curve, depth)
    tree.insert(get_index(curve, bytes(32), depth), concat(bytes(32), bytes(32), 0))
    initial = tree.root
    x, y = bytes(range(32)), bytes([0xEE]) * 32
    ix, iy = get_index(curve, x, depth), get_index(curve, y, depth)
    ups = [Append(x, bytes([1]) * 32, tree.lookup_path(ix))]
    tree.insert(ix, ups[-1].leaf_new)
    ups.append(Append(y, bytes([2]) * 32, tree.lookup_path(iy)))
    tree.insert(iy, ups[-1].leaf_new)
    ups.append(Update(x, 0, bytes([1]) * 32, bytes([3]) * 32, tree.lookup_path(ix)))
    tree.insert(ix, ups[-1].leaf_new)
    return initial, tree.root, ups


@functools.lru_cache(maxsize=None)
def job_b(curve, chal=True):
    initial, final, ups = updates_b(curve)
    job = VkdJob(curve, initial, final, ups, depth=DEPTH, split=SPLIT)
    if chal:
        job.set_challenges(*CHAL)
    return job


@functools.lru_cache(maxsize=None)
def job_small(curve):
    return VkdJob.random(curve, 4, 16, 2)


@functools.lru_cache(maxsize=None)
def assignments(curve, name):
    """The host assignment bytes of every subcircuit of job A / B."""
    job = {"a": job_a, "b": job_b}[name](curve)
    return [job.assignment_bytes(i) for i in range(job.n)]
