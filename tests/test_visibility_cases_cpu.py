"""What makes tests/test_gpu_visibility_decisions.py meaningful, checked on
the CPU oracle's report alone (no GPU): in every case of visibility_cases.py the
tests the case was built for really decide pairs, both ways; some NCC values
are so close to zero that one wrong sample would flip them; and no decision is
so close to its threshold that the order of a sum could flip it -- so the
device's masks can be asked to be array_equal to the oracle's.

Each case prints one line of tally (pytest -s); profiles/
visibility_cases_tally.txt keeps them."""
import numpy as np
import pytest

import visibility_cases as vc

(NOT_VALID, BORDER, OCCLUDED, ANISOTROPY, NCC_OUTSIDE, NCC_NEGATIVE, VISIBLE,
 VISIBLE_NAN) = range(8)

# The decisions are taken in double on both sides, from the same float inputs;
# what differs is the order of the sums (lanes, pairs of samples, running mean
# against sum / n).  Reordering a sum of at most ~4400 x 3 doubles moves it by
# about n * 2^-53, ~1.5e-12 relative; 1e-9 leaves more than two orders of
# magnitude above that.
MARGIN = 1e-9


def _kinds(rep):
    """The pairs that reach ncc_for_patch's norms, split into flat (ncc = 1 by
    the norm test), exact NaN and normal."""
    n = rep["n"]
    with np.errstate(invalid="ignore"):
        reached = rep["reason"] >= NCC_NEGATIVE
        flat = reached & (rep["norm0"] + rep["norm1"] < 0.001 * n)
        nan = rep["reason"] == VISIBLE_NAN
    return reached, flat, nan, reached & ~flat & ~nan


def _sensitive(rep):
    """NCC-decided pairs with |ncc| < 0.5 / n: about what ONE wrong sample
    moves the value by on uniform u8 noise (a term is ~1 / (4 n) per channel)."""
    _, _, _, normal = _kinds(rep)
    with np.errstate(invalid="ignore"):
        return normal & (np.abs(rep["ncc"]) < 0.5 / np.maximum(rep["n"], 1))


def _ratio_margin(rep):
    got = rep["reason"] >= ANISOTROPY
    return np.abs(rep["ratio"][got] - 8.0).min() / 8.0 if got.any() else np.inf


def _tally(case, reps):
    counts = sum(np.bincount(r["reason"].ravel(), minlength=8) for r in reps)
    normal = [_kinds(r)[3] for r in reps]
    min_ncc = min(np.abs(r["ncc"][m]).min() for r, m in zip(reps, normal))
    return ("tally %-24s sets %d  not_valid %d border %d occluded %d anisotropy %d "
            "ncc_outside %d ncc_negative %d visible %d visible_nan %d  flat %d  "
            "|ncc| < 0.5/n %d  min |ncc| %.3g  min |ratio - 8| / 8 %.3g"
            % ((case.name, len(reps)) + tuple(int(c) for c in counts)
               + (sum(int(_kinds(r)[1].sum()) for r in reps),
                  sum(int(_sensitive(r).sum()) for r in reps), min_ncc,
                  min(_ratio_margin(r) for r in reps))))


@pytest.mark.parametrize("case", vc.CASES, ids=vc.ids(vc.CASES))
def test_case_decides_what_it_was_built_for_and_is_well_conditioned(oracle, case):
    reps = [vc.report(oracle, case, k) for k in range(case.sets)]
    print()
    print(_tally(case, reps))
    surf = vc.geometry(case)["surf"]
    for k, rep in enumerate(reps):
        # the report is the same function as orc_topology_subviews: its reasons
        # rebuild the masks of the entry the GPU test compares with
        assert np.array_equal(rep["mask"], vc.oracle_mask(oracle, case, k))
        assert rep["reason"].shape == (surf["npx"] * surf["npy"], case.n_subs)
        assert (rep["reason"] != NOT_VALID).all()          # every patch takes part

    count = lambda reason: sum(int((r["reason"] == reason).sum()) for r in reps)  # noqa: E731
    negative, visible = count(NCC_NEGATIVE), count(VISIBLE)

    # ---- every reason the family is built for has pairs
    if case.family in ("noise", "channels"):
        assert negative >= 200 and visible >= 200
        assert 0.25 <= negative / (negative + visible) <= 0.75
    if case.family == "anisotropy":
        assert count(ANISOTROPY) >= 30
    if case.family == "outside":
        assert count(NCC_OUTSIDE) >= 15
    if case.family == "bands":
        flat_block, zero_block = vc.band_blocks(case)
        for rep in reps:
            _, flat, nan, _ = _kinds(rep)
            assert flat.sum() >= 20 and nan.sum() >= 20
            assert (rep["ncc"][flat] == 1.0).all()
            # and they are the blocks' own patches, nobody else's
            for block, kind in ((flat_block, flat), (zero_block, nan)):
                c0, r0, nc, nr = block
                inside = np.zeros((surf["npy"], surf["npx"]), bool)
                inside[r0:r0 + nr, c0:c0 + nc] = True
                assert not kind[~inside.reshape(-1)].any()
    if case.family == "border":
        flags = vc.template_flags(surf)
        assert tuple(np.unique(flags)) == vc.BORDER_TEMPLATES[case.name]
        assert len(vc.BORDER_TEMPLATES[case.name]) > 1
        rep = reps[0]
        sides = 0
        for f in vc.BORDER_TEMPLATES[case.name]:
            of_f = (flags == f)[:, None]
            candidates = int((of_f & (rep["reason"] >= NCC_OUTSIDE)).sum())
            assert candidates > 0
            if candidates >= 50:
                assert (of_f & (rep["reason"] == NCC_NEGATIVE)).any(), f
                assert (of_f & (rep["reason"] == VISIBLE)).any(), f
                sides += f != 31
        assert sides >= 4          # the four side templates are among those
        # templates differ in their number of samples
        assert len(np.unique(rep["n"][rep["reason"] >= NCC_NEGATIVE])) > 1

    # ---- sensitivity
    assert sum(int(_sensitive(r).sum()) for r in reps) >= 10

    # ---- conditioning
    for rep in reps:
        n = rep["n"].astype(float)
        reached, flat, nan, normal = _kinds(rep)
        assert (rep["n"][reached] > 0).all()
        assert (rep["norm0"][flat] + rep["norm1"][flat] < 0.0005 * n[flat]).all()
        assert (rep["norm1"][nan] == 0).all() and (rep["norm0"][nan] > 0).all()
        n0, n1, m = rep["norm0"][normal], rep["norm1"][normal], n[normal]
        assert (n0 > 0.01 * np.sqrt(m)).all() and (n1 > 0.01 * np.sqrt(m)).all()
        assert (n0 + n1 > 0.002 * m).all()
        assert (np.abs(rep["ncc"][normal]) >= MARGIN).all()
        assert np.isfinite(rep["ncc"][normal]).all()
        assert _ratio_margin(rep) >= MARGIN
        # a pair that stopped earlier carries no later figure
        early = rep["reason"] < ANISOTROPY
        assert np.isnan(rep["ratio"][early]).all() and np.isnan(rep["ncc"][early]).all()
        outside = rep["reason"] == NCC_OUTSIDE
        assert (rep["ncc"][outside] == -1.0).all() and np.isnan(rep["norm0"][outside]).all()
        assert (rep["ratio"][rep["reason"] == ANISOTROPY] > 8.0).all()
        assert (rep["ratio"][rep["reason"] > ANISOTROPY] <= 8.0).all()


def test_the_case_list_has_every_family_and_scale():
    assert [c.scale for c in vc.NOISE] == list(range(7))
    assert all(c.channels == (3,) * (c.n_subs + 1) for c in vc.NOISE)
    assert {c.channels for c in vc.CHANNELS} == {(1, 1, 1, 1, 1), (3, 1, 1, 1, 1),
                                                 (1, 3, 3, 3, 3), (3, 1, 3, 1, 3)}
    assert all(c.scale == 2 for c in vc.CHANNELS)
    assert sorted(c.scale for c in vc.BANDS) == [2, 4]
    assert sorted((c.scale, c.w, c.h) for c in vc.BORDER) == [(0, 97, 80), (1, 160, 129),
                                                             (1, 161, 128)]
    assert sorted((c.scale, c.w, c.h) for c in vc.OUTSIDE) == [(0, 64, 48), (1, 48, 40),
                                                              (1, 64, 48), (2, 64, 48)]
    assert sorted(c.scale for c in vc.ANISOTROPY) == [2, 4, 6]
    for case in vc.CASES:
        imgs = vc.images(case)
        assert len(imgs) == case.n_subs + 1
        for img, c in zip(imgs, case.channels):
            assert img.dtype == np.uint8
            assert img.shape == ((case.h, case.w, 3) if c == 3 else (case.h, case.w))
        if case.sets > 1:
            assert not np.array_equal(imgs[0], vc.images(case, 1)[0])
        assert np.array_equal(imgs[1], vc.images(case)[1])      # seeded


def test_a_flat_block_never_lies_under_a_textured_main_patch():
    """A constant, non-zero neighbour region against a textured main patch
    would make norm1 rounding noise and the NCC's sign undefined: the blocks'
    footprints are only as large as the blocks' own samples."""
    for case in vc.BANDS:
        imgs = vc.images(case)
        flat, zero = vc.band_blocks(case)
        x0, y0, x1, y1 = vc.block_pixels(case, flat)
        assert (imgs[0][y0:y1, x0:x1] == vc.FLAT_BYTE).all()
        zx0, zy0, zx1, zy1 = vc.block_pixels(case, zero)
        assert imgs[0][zy0:zy1, zx0:zx1].std() > 60          # the main view stays noise there
        for j in range(case.n_subs):
            f = vc.block_footprint(case, flat, j)
            z = vc.block_footprint(case, zero, j)
            assert not (f & z).any()
            assert (imgs[1 + j][f] == vc.FLAT_BYTE).all() and (imgs[1 + j][z] == 0).all()
            # a footprint is the block's size plus a few pixels, not a band
            assert f.sum() <= 1.5 * (x1 - x0 + 4) * (y1 - y0 + 4)
