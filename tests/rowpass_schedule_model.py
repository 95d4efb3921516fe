"""A host model of the row pass's deferred-C schedule (k_rowpass_v2<.., PAIR, DEFER_C>, dmf_kernels_rowpass2.hip).

`wave_program(nk, wave)` writes out, for a workgroup of four waves that owns `nk` 16-row blocks, the steps one wave takes in
the kernel's order, with the same index arithmetic as the kernel: tile stores (the counts into a tile set, x as bytes into a
ring slot), phases A, the two barriers of a cycle, phase B, the deferred phases C, the drain.  `check(nk)` then walks the
four programs barrier interval by barrier interval, keeps track of what every count tile, ring slot and ubuf set holds, and
asserts what the hand-over rests on:

  * every wave runs phase C of every block exactly once, in block order;
  * only behind a barrier that follows that block's phase B, and with that block's u in the ubuf set it reads;
  * from a ring slot that holds that block's x (so: not overwritten by a later tile store before its last reader), as
    phase A finds its block in the tile set and the ring slot it reads;
  * no ubuf set is written in a barrier interval in which another wave reads or writes it;
  * every wave meets the same number of barriers.

A wrong hand-over on the device is a hang or silent garbage; here it is an assertion.  Plain Python, no GPU.

The module is also the one Python statement of the row pass's launch rule (rowpass_v2_plan, dmf_kernels_rowpass2.hip), written
from the rules alone: `plan(...)` answers wave count, grid, blocks per workgroup, LDS bytes and schedule, `plan_text(...)` what
dmf_u_phase_describe must say of it (tests/test_rowpass_plan_host.py holds the two together over a grid of shapes), and the
GPU tests ask `schedule`, `runs_deferred`, `blocks_per_workgroup` and `expected_counts` instead of restating any of it."""

NW = 4           # waves of a workgroup on this schedule
RING_PAIRS = 3   # pairs of blocks a wave's x ring holds
UBUF_PAIRS = 3   # pairs of blocks the ubuf sets hold

SCHEDULES = ("one", "pair", "deferred", "bytes")  # each a form of the one before
CU_LDS, CUS = 160 * 1024, 256
TILE_V, TILE_COUNTS, TILE_BYTES = 16 * 66 * 8, 16 * 72 * 2, 1024  # a column group of a block: V (f64), u16 counts (padded rows), the byte image
RING = 2 * RING_PAIRS * 16 * 64                                   # a wave's x ring on the deferred-C schedule


def lds_bytes(S, n_u, n_iter2, x16, schedule="one"):
    """Dynamic LDS of a workgroup: the momentum table, the ubuf sets, the partial-sum slots and the wave sums, then per wave
    its tile sets (V and counts; x and counts on X16; counts alone, x in the ring, with phase C deferred)."""
    nw = (S + 63) // 64
    maxw = 4 if nw <= 4 else 8
    level = SCHEDULES.index(schedule)
    nset = 2 if level >= 1 else 1
    nub = 2 * UBUF_PAIRS if level >= 2 else nset
    nv = n_u * ((n_u + 2) & ~1)
    doubles = ((n_iter2 + 1) & ~1) + nub * 16 * n_u + nset * maxw * nv * 16 + maxw
    tile = TILE_BYTES if level == 3 else TILE_COUNTS if level == 2 else 2 * TILE_COUNTS if x16 else TILE_V + TILE_COUNTS
    return 8 * doubles + nset * nw * tile + (nw * RING if level >= 2 else 0)


def plan(N, S, n_c, n_u, n_iter2=20, x16=True, max_count=255, pair=True, defer_c=True, bytes_=True):
    """The launch plan of k_rowpass_v2 for a problem with integer count copies, or None where the kernel does not take the
    shape.  pair / defer_c / bytes_: the context's three switches."""
    nw = (S + 63) // 64
    if not (N >= 1 and 2 <= S <= 512 and 0 <= n_c <= 16 and 1 <= n_u <= 4):
        return None
    maxw = 4 if nw <= 4 else 8
    wg_cap = (80 if maxw == 4 else 160) * 1024
    if lds_bytes(S, n_u, n_iter2, False) > wg_cap:   # (asked of the V form, the largest)
        return None
    per_cu = 1 if nw > 4 else 8 // nw                # two waves per SIMD
    schedule = "one"
    if pair and x16 and 2 <= nw <= 4 and per_cu * lds_bytes(S, n_u, n_iter2, True, "pair") <= CU_LDS:
        schedule = "pair"
        spills = (n_c + 3) // 4 == 4 and n_u >= 3    # the two instances that are not built
        whole = (lds_bytes(S, n_u, n_iter2, True, "deferred") + 2047) & ~2047   # the LDS is handed out in 2 KB pieces
        if defer_c and max_count <= 255 and nw == NW and not spills and per_cu * whole <= CU_LDS:
            schedule = "bytes" if bytes_ else "deferred"
    nblk = (N + 15) // 16
    grid = min(nblk, CUS * per_cu)
    lds = lds_bytes(S, n_u, n_iter2, x16, schedule)
    return {"nkc": (n_c + 3) // 4, "nw": nw, "maxw": maxw, "grid": grid, "lds": lds, "raise": int(lds > 48 * 1024),
            "blocks": (nblk // grid, (nblk + grid - 1) // grid), "schedule": schedule, "x16": x16, "tail": N % 16}


def plan_text(N, S, n_c, n_u, n_iter2=20, **kw):
    """What dmf_u_phase_describe (route solver) answers where the row pass runs: the rowpass= text of dmf_select_describe,
    then the plan.  None where plan() is."""
    g = plan(N, S, n_c, n_u, n_iter2, **kw)
    if g is None:
        return None
    return (f"k_rowpass_v2<{g['nkc']},{n_u}> nw={g['nw']} grid={g['grid']} tail={g['tail']}{' x16' if g['x16'] else ''} "
            f"maxw={g['maxw']} {g['schedule']} nw={g['nw']} grid={g['grid']} lds={g['lds']} raise={g['raise']} "
            f"blocks/wg={g['blocks'][1]}")


def schedule(S, n_c, n_u, n_iter2=20, **kw):
    return plan(16, S, n_c, n_u, n_iter2, **kw)["schedule"]


def schedule_in_text(text):
    """The schedule word of a u_phase_describe text, None where the text is not the row pass's."""
    return text.split(" maxw=")[1].split()[1] if text.startswith("k_rowpass_v2<") else None


def expected_counts(word, total):
    """(launches, paired, deferred, from bytes) as the solver's counters must show them after `total` launches on the schedule
    `word` (None: the row pass does not run at all)."""
    if word is None:
        return (0, 0, 0, 0)
    return tuple(total if SCHEDULES.index(word) >= i else 0 for i in range(4))


def byte_images_wanted(S, x16, max_count):
    """Whether a problem carries the byte images (rowpass_v2_byte_images_wanted): where some plan of it can read them."""
    return x16 and max_count <= 255 and (S + 63) // 64 == NW


def blocks_per_workgroup(N, S):
    """(fewest, most) blocks a workgroup of the row pass owns: block b goes to workgroup b % grid."""
    return plan(N, S, 0, 1)["blocks"]


def runs_deferred(S, n_c, n_u, n_iter2, max_count, x16=True, pair=True, defer_c=True):
    """Whether a solver's row pass runs the deferred-C schedule, on u16 counts or on bytes."""
    return schedule(S, n_c, n_u, n_iter2, x16=x16, max_count=max_count, pair=pair, defer_c=defer_c) in ("deferred", "bytes")


def wave_program(nk, wave):
    """The steps of one wave, in program order.  Blocks are numbered 0 .. nk - 1 within the workgroup, pair p = blocks
    2 p, 2 p + 1.  Steps: ("store", tile set, ring slot, block), ("A", block, tile set, ring slot), ("barrier", name),
    ("B", block, ubuf set), ("C", block, ring slot, ubuf set)."""
    ops = []

    def phase_c_ring(pp, b01):
        ops.append(("C", 2 * pp + b01, 2 * (pp % 3) + b01, 2 * (pp % 3) + b01))

    for s in range(0, nk, 2):
        has2 = s + 1 < nk
        cyc = s >> 1
        b_role = (wave >> 1) == (cyc & 1)
        rs0 = 2 * (cyc % 3)
        ops.append(("store", 0, rs0, s))
        if has2:
            ops.append(("store", 1, rs0 + 1, s + 1))
        bset = 1 if (has2 and wave == (s + 1) % NW) else 0
        my_turn = bset == 1 or wave == s % NW
        ops.append(("A", s, 0, rs0))
        if has2:
            ops.append(("A", s + 1, 1, rs0 + 1))
        ops.append(("barrier", "X"))
        if my_turn:
            assert b_role
            ops.append(("B", s + bset, rs0 + bset))
        if not b_role:
            for pp in range(max(cyc - 2, 0), cyc):
                phase_c_ring(pp, 0)
                phase_c_ring(pp, 1)
        ops.append(("barrier", "Y"))
    if nk > 0:
        last = (nk - 1) >> 1
        lone = (nk & 1) != 0
        first = last if ((wave >> 1) != (last & 1) or last == 0) else last - 1
        for pp in range(first, last + 1):
            phase_c_ring(pp, 0)
            if pp < last or not lone:
                phase_c_ring(pp, 1)
    return ops


def check(nk):
    """Walks the four waves' programs and asserts the schedule's properties; returns the number of barriers per wave."""
    progs = [wave_program(nk, w) for w in range(NW)]
    # barrier intervals: interval[w][k] = the steps of wave w between its k-th and (k + 1)-th barrier
    intervals = []
    for ops in progs:
        cur, out = [], []
        for op in ops:
            if op[0] == "barrier":
                out.append(cur)
                cur = []
            else:
                cur.append(op)
        out.append(cur)
        intervals.append(out)
    n_bar = [len(iv) - 1 for iv in intervals]
    assert len(set(n_bar)) == 1, ("barrier counts differ", nk, n_bar)
    names = [[op[1] for op in ops if op[0] == "barrier"] for ops in progs]
    assert all(n == names[0] for n in names), ("barrier sequences differ", nk)

    tile = [[None, None] for _ in range(NW)]                   # block whose counts a wave's tile set holds
    ring = [[None] * (2 * RING_PAIRS) for _ in range(NW)]      # block whose x a wave's ring slot holds
    ubuf = [None] * (2 * UBUF_PAIRS)                           # block whose u an ubuf set holds
    b_done = {}                                                # block -> interval its phase B ran in
    a_done = [set() for _ in range(NW)]
    c_seen = [[] for _ in range(NW)]
    for k in range(n_bar[0] + 1):
        written, read = {}, {}
        for w in range(NW):
            for op in intervals[w][k]:
                if op[0] == "store":
                    tile[w][op[1]] = op[3]
                    ring[w][op[2]] = op[3]
                elif op[0] == "A":
                    assert tile[w][op[2]] == op[1] and ring[w][op[3]] == op[1], ("phase A without its tile", nk, w, k, op)
                    a_done[w].add(op[1])
                elif op[0] == "B":
                    blk, uset = op[1], op[2]
                    assert blk not in b_done, ("phase B twice", nk, blk)
                    assert w == blk % NW, ("phase B on the wrong wave", nk, w, blk)
                    written.setdefault(uset, []).append((w, blk))
                elif op[0] == "C":
                    blk, slot, uset = op[1], op[2], op[3]
                    assert ring[w][slot] == blk, ("phase C reads a ring slot that holds another block", nk, w, k, op, ring[w])
                    assert blk in b_done and b_done[blk] < k, ("phase C without a barrier behind phase B", nk, w, k, op)
                    assert ubuf[uset] == blk, ("phase C reads an ubuf set that holds another block", nk, w, k, op, ubuf)
                    read.setdefault(uset, []).append((w, blk))
                    c_seen[w].append(blk)
        for uset, ws in written.items():
            assert len(ws) == 1, ("two phases B write one ubuf set in one interval", nk, k, uset, ws)
            assert uset not in read, ("an ubuf set written while it is read", nk, k, uset, ws, read[uset])
        for uset, ws in written.items():
            # phase B needs every wave's partial sums: phase A of the block, before the barrier in front of this interval
            blk = ws[0][1]
            assert all(blk in a_done[w] for w in range(NW)), ("phase B before every phase A", nk, k, blk)
            ubuf[uset] = blk
            b_done[blk] = k
    assert sorted(b_done) == list(range(nk)), ("phase B missing", nk, sorted(b_done))
    for w in range(NW):
        assert c_seen[w] == list(range(nk)), ("phase C not once per block in block order", nk, w, c_seen[w])
    return n_bar[0]


def pending_at_drain(nk, wave):
    """Blocks whose phase C a wave runs in the drain (behind the last barrier)."""
    ops = wave_program(nk, wave)
    last_bar = max((i for i, op in enumerate(ops) if op[0] == "barrier"), default=-1)
    return [op[1] for op in ops[last_bar + 1:] if op[0] == "C"]
