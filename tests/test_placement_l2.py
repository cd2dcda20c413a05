"""CPU: placement of L2 sources.  plan(..., group_l2=True) lets the "l2" sources of one encoder share search units and be cut into
row slices like ip / cosine ones (one rr_flat_search_segments_l2 per rank and group); the default keeps every piece of an L2
source a unit of its own, as before.  Host logic only."""
from ragroute_amd import placement as P


def wikipedia(rows=None):
    """The reference's wikipedia federation: ten sources behind one DPR question encoder (config.py:35, 59-70), width 768, L2."""
    rows = rows or [2_100_000 + 1_000 * i for i in range(10)]
    return [P.Source(s, n, 768, "facebook/dpr-question_encoder-single-nq-base", "l2", "fp16", f"cluster{s}") for s, n in enumerate(rows)]


def covered(pl, fed):
    """every row of every source exactly once"""
    for src in fed:
        at = 0
        for sl in pl.slices_of(src.sid):
            assert sl.row_begin == at and sl.n_rows >= 0
            at += sl.n_rows
        assert at == src.rows, (src.sid, at, src.rows)
    assert sum(sl.n_rows for units in pl.ranks for u in units for sl in u.slices) == sum(s.rows for s in fed)


def test_grouped_l2_sources_are_covered_once_share_units_and_cut_on_256_rows():
    fed = wikipedia()
    for G in (1, 2, 4, 8):
        pl = P.plan(fed, G, group_l2=True)
        covered(pl, fed)
        for units in pl.ranks:
            assert len(units) == 1, "the pieces of one L2 group on a rank form one unit"
            assert units[0].group == fed[0].group and units[0].group[2] == "l2"
            ids = [sl.id_offset for sl in units[0].slices]
            assert ids == sorted(ids), "ascending id offsets: ties by ascending global id"
        cuts = [sl for units in pl.ranks for u in units for sl in u.slices if sl.row_begin > 0]
        assert len(cuts) <= G - 1 and all(sl.row_begin % P.SLICE_ALIGN == 0 for sl in cuts)
        if G in (4, 8):                     # ten sources do not divide over 4 or 8 ranks: without cuts a rank would carry 3 against 2
            assert cuts
        assert pl.imbalance < 1.02
        assert pl.slots == 1


def test_grouped_l2_keeps_other_groups_apart():
    """L2 and inner-product sources of the same encoder and width never share a unit (their scores cannot be merged in one search),
    nor do L2 sources of different encoders."""
    fed = wikipedia([300_000, 200_000, 100_000]) + [P.Source(3, 250_000, 768, "facebook/dpr-question_encoder-single-nq-base", "ip"),
                                                    P.Source(4, 150_000, 768, "other", "l2")]
    pl = P.plan(fed, 2, group_l2=True)
    covered(pl, fed)
    for units in pl.ranks:
        for u in units:
            assert len({pl.sources[sl.sid].group for sl in u.slices}) == 1
    assert any(u.segmented and u.group[2] == "l2" for units in pl.ranks for u in units)


def test_the_default_plan_is_unchanged():
    """group_l2=False (the default) is the layout from before the segmented L2 search: every piece of an L2 source is a unit of its
    own, whatever else the federation holds.  Stated twice: by construction (one slice per L2 unit), and against a planner whose
    L2 sources carry distinct encoder keys - the same pouring, with grouping made impossible - on a mixed federation."""
    fed = wikipedia([900_000, 100_000, 2_000_000, 70_000]) + [P.Source(4, 500_000, 1024, "uae"), P.Source(5, 300_000, 1024, "uae")]
    for G in (1, 3, 4):
        pl = P.plan(fed, G)
        covered(pl, fed)
        assert P.plan(fed, G, group_l2=False).describe() == pl.describe()
        for units in pl.ranks:
            for u in units:
                if u.group[2] == "l2":
                    assert len(u.slices) == 1
        grouped = P.plan(fed, G, group_l2=True)
        assert sum(len(u) for u in grouped.ranks) < sum(len(u) for u in pl.ranks)
        # ip / cosine federations do not depend on the switch at all
        ip = [P.Source(s.sid, s.rows, s.dim, s.encoder, "ip") for s in fed]
        assert P.plan(ip, G, group_l2=True).describe() == P.plan(ip, G).describe()


# describe() of plan(fed, 3) for the federation below, as the planner laid it out before group_l2 existed (recorded from that version)
DEFAULT_PLAN_G3 = [
    {"rank": 0, "predicted_ms": 0.6778, "units": [
        {"encoder": "facebook/dpr-question_encoder-single-nq-base", "dim": 768, "slices": [{"source": "cluster0", "row_begin": 0, "n_rows": 900000}]},
        {"encoder": "facebook/dpr-question_encoder-single-nq-base", "dim": 768, "slices": [{"source": "cluster1", "row_begin": 0, "n_rows": 100000}]},
        {"encoder": "facebook/dpr-question_encoder-single-nq-base", "dim": 768, "slices": [{"source": "cluster2", "row_begin": 0, "n_rows": 268288}]}]},
    {"rank": 1, "predicted_ms": 0.6777, "units": [
        {"encoder": "facebook/dpr-question_encoder-single-nq-base", "dim": 768, "slices": [{"source": "cluster2", "row_begin": 268288, "n_rows": 1731712}]}]},
    {"rank": 2, "predicted_ms": 0.5752, "units": [
        {"encoder": "facebook/dpr-question_encoder-single-nq-base", "dim": 768, "slices": [{"source": "cluster3", "row_begin": 0, "n_rows": 70000}]},
        {"encoder": "uae", "dim": 1024, "slices": [{"source": "a", "row_begin": 0, "n_rows": 500000}, {"source": "b", "row_begin": 0, "n_rows": 300000}]}]},
]


def test_the_default_plan_equals_the_recorded_layout():
    fed = wikipedia([900_000, 100_000, 2_000_000, 70_000]) + [P.Source(4, 500_000, 1024, "uae", name="a"), P.Source(5, 300_000, 1024, "uae", name="b")]
    assert P.plan(fed, 3).describe() == DEFAULT_PLAN_G3
    assert P.plan(fed, 3, group_l2=False).describe() == DEFAULT_PLAN_G3
    grouped = P.plan(fed, 3, group_l2=True)
    assert grouped.describe() != DEFAULT_PLAN_G3 and max(grouped.predicted_ms) <= max(P.plan(fed, 3).predicted_ms) + 1e-9
