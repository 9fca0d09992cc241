"""Tracer.Read of traceloop (pkg/gadgets/traceloop/tracer/tracer.go:246-545) restated row by row,
exactly as the Go is written: per container three maps of slices keyed by the monotonic timestamp
(:313-317, :338-345), the publishing loop over the enter map with its deletes (:362-457), the two
loops over what is left (:468-530) and the sort by event time (:533-535).  Rows are named by their
index in their stream, so that the result can be compared with igx_traceloop_join's columns.

The reference's order among events of equal time is map iteration followed by an unstable sort,
i.e. undefined; here ties go ascending by syscall row (the event's own row: the enter row, or the
exit row of an incomplete exit), the order include/igx.h chooses.  Syscall names and declarations
are the gadget's business (gadgets.TraceloopTracer); the three syscalls without an exit are given
by number.  Test infrastructure only."""

NO = 0xFFFFFFFF
NR_X86_64 = (60, 231, 15)     # exit, exit_group, rt_sigreturn
NR_ARM64 = (93, 94, 139)
COMPLETE, INCOMPLETE_ENTER, INCOMPLETE_EXIT = 0, 1, 2
ARGS = 6


def _aslist(c):
    if c is None:
        return None
    return c.tolist() if hasattr(c, "tolist") else list(c)


def read_one(rows, conts, nr=NR_X86_64):
    """One container's Read.  rows: (row, mono_ts, sort_ts, typ, id, pid) in read order; conts:
    (row, mono_ts, index) in read order.  Returns events (sort_ts, row, exit, class, [cont] * 6),
    unsorted, in the order the loops append them with maps iterated in insertion order."""
    cont_map, enter_map, exit_map = {}, {}, {}
    for r in rows:
        typ = r[3]
        if typ == 0:
            type_map = enter_map
        elif typ == 1:
            type_map = exit_map
        else:
            continue                                            # :304-311
        if r[1] not in type_map:
            type_map[r[1]] = []
        type_map[r[1]].append(r)
    for c in conts:
        if c[1] not in cont_map:
            cont_map[c[1]] = []
        cont_map[c[1]].append(c)

    events = []
    for ts, enters in list(enter_map.items()):                  # :362
        for e in enters:                                        # :363 (ranges over the slice it took)
            params = [NO] * ARGS
            for i in range(ARGS):                               # :390 (the declared ones are a prefix)
                for c in cont_map.get(ts, []):                  # :400-407
                    if c[2] == i:
                        params[i] = c[0]
                        break
            cont_map.pop(ts, None)                              # :415
            if e[4] in nr:                                      # :418
                enter_map.pop(ts, None)
                events.append((e[2], e[0], NO, COMPLETE, params))
                continue
            exits = exit_map.get(ts)                            # :431
            if exits is None:
                continue
            for x in exits:                                     # :438
                if e[4] != x[4] or e[5] != x[5]:
                    continue
                enter_map.pop(ts, None)                         # :445-446
                exit_map.pop(ts, None)
                events.append((e[2], e[0], x[0], COMPLETE, params))
                break
    for enters in enter_map.values():                           # :468
        for e in enters:
            events.append((e[2], e[0], NO, INCOMPLETE_ENTER, [NO] * ARGS))
    for exits in exit_map.values():                             # :500
        for x in exits:
            events.append((x[2], x[0], NO, INCOMPLETE_EXIT, [NO] * ARGS))
    return events


def join(mono_ts, sort_ts, typ, id, pid, valid=None, mntns=None, c_mono_ts=(), c_index=(), c_valid=None,
         c_mntns=None, nr=NR_X86_64):
    """The columns of igx_traceloop_join: (ev_row, ev_exit, ev_class, ev_cont) as lists, ev_cont
    flat with six entries per event.  mntns None: one container."""
    mono_ts, sort_ts, typ, id, pid = (_aslist(c) for c in (mono_ts, sort_ts, typ, id, pid))
    valid, mntns, c_valid, c_mntns = (_aslist(c) for c in (valid, mntns, c_valid, c_mntns))
    c_mono_ts, c_index = _aslist(c_mono_ts), _aslist(c_index)
    per = {}
    for i in range(len(mono_ts)):
        if valid is not None and not valid[i]:
            continue
        k = None if mntns is None else mntns[i]
        per.setdefault(k, ([], []))[0].append((i, mono_ts[i], sort_ts[i], typ[i], id[i], pid[i]))
    for j in range(len(c_mono_ts)):
        if c_valid is not None and not c_valid[j]:
            continue
        k = None if c_mntns is None else c_mntns[j]
        per.setdefault(k, ([], []))[1].append((j, c_mono_ts[j], c_index[j]))
    events = []
    for rows, conts in per.values():
        events += read_one(rows, conts, nr)
    events.sort(key=lambda e: (e[0], e[1]))
    ev_cont = [c for e in events for c in e[4]]
    return [e[1] for e in events], [e[2] for e in events], [e[3] for e in events], ev_cont
