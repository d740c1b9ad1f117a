"""The read-selection rule (include/strkit_amd.h) in a dozen lines of dict-and-loop Python over the (name, flag)
list of one locus: the oracle of the select tests.  Names are bytes or str; equality is Python's."""


def select(items, rules, max_reads):
    """-> (reason per item, status per item, number kept)."""
    status = {}
    for name, flag in items:
        status[name] = status.get(name, 0) | (2 if flag & 0x800 else 1)
    reasons, seen, survivors = [], set(), 0
    for name, flag in items:
        if rules & 1 and flag & 0x800:
            reasons.append(1)
        elif rules & 2 and flag & 0x100:
            reasons.append(2)
        elif rules & 4 and name in seen:
            reasons.append(3)
        else:
            reasons.append(0 if survivors < max_reads else 4)
            survivors += 1
        if reasons[-1] not in (1, 2):
            seen.add(name)
    return reasons, [status[name] for name, _ in items], min(survivors, max_reads)


def survivors(items, rules):
    """The items that no flag skip and no duplicate rule removes (what the cap then counts)."""
    return sum(r == 0 for r in select(items, rules, 1 << 40)[0])
