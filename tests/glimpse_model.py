"""The glimpse memory's rule (include/agx_glimpse.h) on top of tests/history_model.py's HistoryModel: which glimpses of a sample
(n, k) are taken for P glimpses.  Bookkeeping only, no pixels."""


def taken_glimpses(model, n, k, glimpses):
    """The list of i in 0 .. P - 1 whose glimpse (n, k - i) is taken: i <= age[k] (no CLEAR between the two appends) and
    (n, k - i) is itself a valid sample.  Empty for an invalid sample (glimpse 0 is (n, k) itself)."""
    if not model.valid(n, k):
        return []
    age = int(model.age[k % model.T, n])
    return [i for i in range(int(glimpses)) if i <= age and model.valid(n, k - i)]


def taken_count(model, n, k, glimpses):
    """What the kernel reports: the number of glimpses taken.  They are always 0 .. count - 1 (asserted)."""
    got = taken_glimpses(model, n, k, glimpses)
    assert got == list(range(len(got))), "taken glimpses are not a prefix"
    return len(got)


def sample_class(model, n, k, glimpses):
    """"invalid", "full" (all P taken), "clear" (the episode is younger than P appends), or "evicted" (an older glimpse of
    the same episode is no longer retained)."""
    c = taken_count(model, n, k, glimpses)
    if c == 0:
        return "invalid"
    if c == int(glimpses):
        return "full"
    age = int(model.age[k % model.T, n])
    return "clear" if c == age + 1 else "evicted"
