"""Launch planning of the batched Textcoder AR decode (CubenetTextcoder.inference_batch).  Plain Python: importable without the library.

A launch of the split AR kernel holds `members` workgroups per row for as long as its LONGEST row runs, and all of them must be co-resident,
so a launch takes at most CUs // members rows.  Rows are handed out longest first: rows of similar length share a launch, and the short
launches come last."""


def plan_ar_launches(steps, max_rows):
    """steps: AR steps per row; max_rows: the row cap of one launch (>= 1).  -> list of row-index lists, one per launch: every row with
    steps > 0 exactly once, longest first (ties in row order), at most max_rows rows per launch; rows with zero steps appear in none."""
    max_rows = int(max_rows)
    if max_rows < 1:
        raise ValueError('plan_ar_launches: max_rows must be at least 1 (got %r)' % (max_rows,))
    steps = [int(s) for s in steps]
    if any(s < 0 for s in steps):
        raise ValueError('plan_ar_launches: negative step count')
    order = sorted((b for b, s in enumerate(steps) if s > 0), key=lambda b: (-steps[b], b))
    return [order[i:i + max_rows] for i in range(0, len(order), max_rows)]
