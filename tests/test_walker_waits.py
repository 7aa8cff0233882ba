"""What the walker's waves wait for between two row groups (build container, no GPU).

`s_waitcnt vmcnt` counts vector loads and stores together, in order, and the compiler can only count what every path
issues.  walk_strip<true> requests the next group's four pixel rows and then writes up to four rows of level l + 1: with
the stores behind branches, the only wait that guarantees the rows was vmcnt(0), which also waits for the write-through
acknowledgement of every store.  The stores are therefore issued on every path (those without an output row are dropped
by the buffer range check), and this test reads the compiled kernel to see that it stays so: in the loop over row groups
that holds the `sc1` pyramid stores (the four copies of the group body, one after the other), every path from one
group's stores to the next group's that does not flush issues the same number of stores, and none holds a vmcnt(0)."""
import os
import re
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))

import asm_audit  # noqa: E402

pytestmark = pytest.mark.skipif(asm_audit.hipcc() is None, reason="needs hipcc (cross-compiles without a GPU)")

STORES_PER_GROUP = 4           # RZ_EMIT x 4 in walk_strip's group body
PHASES = 4                     # the group body exists once per position of the group in the 16-row ring


def _k_walk_lines(tmp_path):
    out = str(tmp_path / "orb.s")
    src = os.path.join(asm_audit.CSRC, "orb_kernels.hip")
    r = subprocess.run([asm_audit.hipcc()] + asm_audit.FLAGS + ["-o", out, src], stderr=subprocess.PIPE, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
    lines = open(out).read().split("\n")
    start = next(i for i, ln in enumerate(lines) if re.match(r"^_ZN3msf6k_walk\w*:", ln))
    end = next(i for i in range(start, len(lines)) if "s_endpgm" in lines[i])
    return lines[start + 1:end]


def _blocks(lines):
    """basic blocks of the kernel: name -> (marker line, instructions); a block starts at a label or at the marker of a
    fall-through block and ends with its branches"""
    blocks, order, cur = {}, [], None
    for ln in lines:
        m = re.match(r"^\.(LBB\d+_\d+):(.*)$", ln) or re.match(r"^; %(bb\.\d+):(.*)$", ln)
        if m:
            cur = m.group(1)
            blocks[cur] = [m.group(2), []]
            order.append(cur)
        elif cur is not None:
            blocks[cur][1].append(ln)
    succ = {}
    for i, b in enumerate(order):
        ins = [ln.strip() for ln in blocks[b][1]]
        s = [m.group(1) for ln in ins for m in [re.match(r"s_cbranch_\w+ \.(LBB\d+_\d+)", ln)] if m]
        jump = [m.group(1) for ln in ins for m in [re.match(r"s_branch \.(LBB\d+_\d+)", ln)] if m]
        if jump:
            s += jump
        elif i + 1 < len(order):
            s.append(order[i + 1])
        succ[b] = s
    return blocks, succ


def _is_sc1_store(ln):
    return re.match(r"\s*buffer_store_\w+ .*\bsc1\b", ln) is not None


def test_row_group_stores_are_counted_and_no_full_wait_lies_between_two_groups(tmp_path):
    blocks, succ = _blocks(_k_walk_lines(tmp_path))
    # the loop over row groups of walk_strip<true>: the depth-1 loop whose own blocks hold the sc1 stores
    headers = set()
    for name, (mark, ins) in blocks.items():
        if any(_is_sc1_store(ln) for ln in ins):
            m = re.search(r"in Loop: Header=(BB\d+_\d+) Depth=1\b", mark)
            if m:
                headers.add("L" + m.group(1))
    assert len(headers) == 1, "one loop over row groups holds the pyramid stores: %s" % sorted(headers)
    head = headers.pop()
    own = {head} | {b for b, (mark, _) in blocks.items() if re.search(r"in Loop: Header=%s Depth=1\b" % head[1:], mark)}
    store_blocks = [b for b in own if any(_is_sc1_store(ln) for ln in blocks[b][1])]
    assert sum(sum(_is_sc1_store(ln) for ln in blocks[b][1]) for b in store_blocks) == PHASES * STORES_PER_GROUP

    # paths that do not flush: through the loop's own blocks (the flush's loops are child loops) and through no block
    # with a wave barrier (flush() and flush_out() begin and end with one; the group body has none)
    def hot(b):
        return b in own and not any("; wave barrier" in ln for ln in blocks[b][1])

    # every group's stores stand in one basic block: no path through a group leaves one out
    assert len(store_blocks) == PHASES
    for b in store_blocks:
        assert sum(bool(re.match(r"\s*buffer_store_", ln)) for ln in blocks[b][1]) == STORES_PER_GROUP, b

    def reach(edges):
        """hot blocks reached from the store blocks along `edges`, not walking on through another store block"""
        seen, todo = set(), list(store_blocks)
        while todo:
            for n in edges.get(todo.pop(), ()):
                if hot(n) and n not in seen:
                    seen.add(n)
                    if n not in store_blocks:
                        todo.append(n)
        return seen

    pred = {}
    for b, ss in succ.items():
        for n in ss:
            pred.setdefault(n, []).append(b)
    # the blocks on a path without a flush from one group's stores to the next group's (through the back edge too)
    between = (reach(succ) & reach(pred)) | set(store_blocks)
    assert head in between
    for b in between - set(store_blocks):
        assert not any(re.match(r"\s*(buffer_store|global_store|global_atomic|buffer_atomic)", ln) for ln in blocks[b][1]), \
            "a store on one path between two row groups only (%s): the wait for the queued rows cannot be counted" % b
    waits = sorted(int(m.group(1)) for b in between for ln in blocks[b][1]
                   for m in [re.search(r"s_waitcnt.*vmcnt\((\d+)\)", ln)] if m)
    assert 0 not in waits, "a vmcnt(0) between two row groups waits for the pyramid stores' acknowledgements: %s" % waits
    # per group: the queued rows are waited for at their first use, behind the four stores of the group before
    # (rows 0 and 1 of the queue go to the ring with one LDS write, rows 2 and 3 with the next)
    assert waits == [4] * PHASES + [6] * PHASES, waits
