"""The item fronts of k_n16_fused_u and k_n16_edge_u as the compiler emits them (no GPU: `make isa` cross-compiles pf_n16.hip with the
library's own flags and this test reads the assembly).

The fronts depend on where the compiler puts loads and waits, which the source can only steer: a load whose value is used on one
side of a branch is moved behind that branch, and a scalar load of a kernel argument is waited for where it is used.  The source
steers with preloaded arguments, with uses placed in front of the early exits, with a store that never executes, and with values
pinned in scalar registers (pf_n16.hip: n16_pin, n16_fused_args).  A compiler update that undoes any of it would put
the dependent round trips back without failing any other test; this one fails instead.

Checked: the preload lengths (12 and 14 user scalar registers: the records' address, resp. the region starts and pa_skip's
offset are among them), and in the record path of k_n16_fused_u -- from the count's load to the first ds_bpermute, one
straight-line stretch -- the three record loads and the twelve quads of the weights' ring, no branch, and a single wait on scalar
loads, in front of the quads."""
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "pharmacophore-diffusion_amd", "csrc")


def _functions(path):
    """name -> lines of every kernel of the assembly, and name -> its preload length."""
    body, cur, preload, kd = {}, None, {}, None
    for line in open(path):
        m = re.match(r"^(_Z\w+):", line)
        if m:
            cur = m.group(1); body[cur] = []
            continue
        m = re.match(r"^\s*\.amdhsa_kernel (\w+)", line)
        if m:
            kd, cur = m.group(1), None
        m = re.match(r"^\s*\.amdhsa_user_sgpr_kernarg_preload_length (\d+)", line)
        if m and kd:
            preload[kd] = int(m.group(1))
        if cur is not None:
            body[cur].append(line.rstrip("\n"))
    return body, preload


def test_record_front_and_preload_lengths(tmp_path):
    out = tmp_path / "pf_n16.s"
    subprocess.run(["make", "-C", CSRC, "-s", "isa", "ARCH=gfx950", f"ISA_OUT={out}"], check=True)
    body, preload = _functions(out)
    fused = [k for k in body if "k_n16_fused_u" in k]
    edge = [k for k in body if "k_n16_edge_u" in k]
    assert len(fused) == 1 and len(edge) == 1, (fused, edge)
    assert preload[fused[0]] == 12 and preload[edge[0]] == 14, (preload[fused[0]], preload[edge[0]])

    lines = body[fused[0]]
    # the count of the record path is the kernel's only single-dword buffer load
    start = [i for i, l in enumerate(lines) if re.search(r"\bbuffer_load_dword v\d+,", l)]
    assert len(start) == 1, start
    end = next(i for i in range(start[0], len(lines)) if "ds_bpermute_b32" in lines[i])
    front = lines[start[0]:end]
    assert not [l for l in front if re.search(r"\bs_cbranch|\bs_branch|^\.LBB", l)], "a branch stands inside the record front"
    records = [i for i, l in enumerate(front) if "global_load_dwordx4" in l]
    quads = [i for i, l in enumerate(front) if "buffer_load_dwordx4" in l]
    waits = [i for i, l in enumerate(front) if "s_waitcnt" in l and "lgkmcnt" in l]
    assert len(records) == 3 and len(quads) == 12, (len(records), len(quads))
    assert len(waits) == 1 and max(records) < waits[0] < min(quads), (records, waits, quads[:1])
    # the records are waited for by their own counter only, behind the quads
    vm = [i for i, l in enumerate(front) if "s_waitcnt" in l and "vmcnt" in l]
    assert vm and min(vm) > max(quads), (vm, quads[-1])
