"""The K loops of the fused pair kernels keep their weight ring in flight: no short vmcnt wait inside them.

build.py keeps the device assembly of qvc_conv_f16.hip and qvc_conv_bf16.hip next to the resource remarks.  In every
shipped rbpair_kernel instantiation, every innermost loop that holds MFMAs (the GEMM1 and the GEMM2 K loop) is read
from that assembly; inside them no `s_waitcnt vmcnt(N)` may have N < 4.  The ring runs three k-steps ahead at two
16-byte loads per k-step (MF = 2), so a wait that only retires the k-step about to be consumed leaves 6-7 loads
outstanding; 4 still means two k-steps in flight.  A guarded prefetch (a wave-uniform branch around the loads) makes
hipcc wait vmcnt(1) and vmcnt(0) directly behind the loads it has just issued, once per group of four k-steps.
"""
import os
import re
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OBJ = os.path.join(ROOT, "quickvc-official_amd", "csrc", "_obj")

# <operand, MF, NF, WM, NWV, stream>: the 4-wave (stage 2) and 8-wave (stage 1) layouts of the shipped config in the
# f16, bf16 and bf16x (bf16 operands, f16 residual stream) modes
SHIPPED = [
    ("qvc_conv_f16.s", "rbpair_kernelIDF16_Li2ELi10ELi4ELi4EDF16_E"),
    ("qvc_conv_f16.s", "rbpair_kernelIDF16_Li2ELi10ELi8ELi8EDF16_E"),
    ("qvc_conv_bf16.s", "rbpair_kernelIDF16bLi2ELi10ELi4ELi4EDF16bE"),
    ("qvc_conv_bf16.s", "rbpair_kernelIDF16bLi2ELi10ELi8ELi8EDF16bE"),
    ("qvc_conv_bf16.s", "rbpair_kernelIDF16bLi2ELi10ELi4ELi4EDF16_E"),
    ("qvc_conv_bf16.s", "rbpair_kernelIDF16bLi2ELi10ELi8ELi8EDF16_E"),
]
MIN_VMCNT = 4


@pytest.fixture(scope="module")
def built():
    """Build (or reuse) the product library: build.py leaves the assembly next to the objects."""
    sys.path.insert(0, ROOT)
    import __graft_entry__ as ge
    ge.build()


def function_body(path, tag):
    """The instruction lines of the one kernel whose mangled name contains `tag`."""
    body, name = None, None
    with open(path) as f:
        for line in f:
            if body is None:
                m = re.match(r"(_Z\w+):", line)
                if m and tag in m.group(1):
                    name, body = m.group(1), []
            else:
                if line.startswith(".Lfunc_end") or line.lstrip().startswith(".end_amdhsa_kernel"):
                    break
                body.append(line.split(";")[0].strip())
    assert body, "kernel %s not found in %s" % (tag, path)
    return name, body


def _blocks(body):
    """Basic blocks of a kernel as (first, last + 1) line ranges, and the successor lists of its control-flow graph."""
    label_at = {m.group(1): i for i, ins in enumerate(body) for m in [re.match(r"(\.LBB\d+_\d+):", ins)] if m}
    is_jump = lambda ins: re.match(r"s_(c?branch\w*|endpgm|setpc\w*)\b", ins)
    starts = sorted({0} | set(label_at.values()) | {i + 1 for i, ins in enumerate(body) if is_jump(ins) and i + 1 < len(body)})
    blocks = [(a, b) for a, b in zip(starts, starts[1:] + [len(body)])]
    index = {a: n for n, (a, _) in enumerate(blocks)}
    succ = []
    for n, (a, b) in enumerate(blocks):
        out = []
        tail = next((ins for ins in reversed(body[a:b]) if ins and not ins.endswith(":")), "")
        m = re.match(r"s_c?branch\w*\s+(\.LBB\d+_\d+)", tail)
        if m:
            out.append(index[label_at[m.group(1)]])
        if not re.match(r"s_(branch|endpgm|setpc\w*)\b", tail) and n + 1 < len(blocks):
            out.append(n + 1)                                         # falls through
        succ.append(out)
    return blocks, succ


def _sccs(nodes, succ):
    """Strongly connected components (Tarjan, iterative) of the graph restricted to `nodes`."""
    nodes = set(nodes)
    idx, low, on, stack, out, count = {}, {}, set(), [], [], 0
    for root in sorted(nodes):
        if root in idx:
            continue
        work = [(root, iter([w for w in succ[root] if w in nodes]))]
        idx[root] = low[root] = count; count += 1; stack.append(root); on.add(root)
        while work:
            v, it = work[-1]
            w = next(it, None)
            if w is None:
                work.pop()
                if work:
                    low[work[-1][0]] = min(low[work[-1][0]], low[v])
                if low[v] == idx[v]:
                    comp = []
                    while True:
                        x = stack.pop(); on.discard(x); comp.append(x)
                        if x == v:
                            break
                    out.append(comp)
            elif w not in idx:
                idx[w] = low[w] = count; count += 1; stack.append(w); on.add(w)
                work.append((w, iter([x for x in succ[w] if x in nodes])))
            elif w in on:
                low[v] = min(low[v], idx[w])
    return out


def innermost_mfma_loops(body):
    """The innermost loops of the kernel that hold at least one MFMA, each as the list of its instruction lines.  A loop
    is a cycle of the control-flow graph (a strongly connected component), not any backward branch: the block
    placement of hipcc jumps backwards into straight-line tail code too.  Loops nested in a component are found by
    cutting the edges into its entry blocks and looking again."""
    blocks, succ = _blocks(body)
    pred = [[] for _ in blocks]
    for n, out in enumerate(succ):
        for w in out:
            pred[w].append(n)

    def loops_in(nodes, succ):
        found = []
        for comp in _sccs(nodes, succ):
            cset = set(comp)
            if len(comp) == 1 and comp[0] not in succ[comp[0]]:
                continue                                              # a single block with no edge to itself: no loop
            entries = {n for n in comp if any(q not in cset for q in pred[n])} or {min(comp)}
            cut = [[w for w in out if not (n in cset and w in entries)] for n, out in enumerate(succ)]
            found += loops_in(comp, cut) or [sorted(comp)]
        return found

    loops = [[ins for n in comp for ins in body[blocks[n][0]:blocks[n][1]]] for comp in loops_in(range(len(blocks)), succ)]
    return [l for l in loops if any(ins.startswith("v_mfma") for ins in l)]


def loop_vmcnt_waits(path, tag):
    name, body = function_body(path, tag)
    out = []
    for loop in innermost_mfma_loops(body):
        waits = []
        for ins in loop:
            if ins.startswith("s_waitcnt"):
                m = re.search(r"vmcnt\((\d+)\)", ins)
                if m:
                    waits.append(int(m.group(1)))
                elif re.match(r"s_waitcnt\s+(0x[0-9a-fA-F]+|\d+)\s*$", ins):     # a raw immediate waits on every counter
                    waits.append(0)
        out.append({"mfma": sum(ins.startswith("v_mfma") for ins in loop),
                    "loads": sum(ins.startswith("global_load") for ins in loop), "vmcnt": waits})
    return name, out


@pytest.mark.parametrize("asm,tag", SHIPPED, ids=[t for _, t in SHIPPED])
def test_pair_k_loops_never_drain_the_weight_ring(built, asm, tag):
    name, loops = loop_vmcnt_waits(os.path.join(OBJ, asm), tag)
    print(name, loops)
    k_loops = [l for l in loops if l["loads"]]                    # the K loops stream weights; both GEMMs have one
    assert len(k_loops) >= 2, (name, loops)
    for l in loops:
        assert all(n >= MIN_VMCNT for n in l["vmcnt"]), (name, l)
    for l in k_loops:
        assert l["vmcnt"], (name, l)                               # a K loop with no vmcnt wait at all would not be the ring we mean
