"""Device-side picture complexity (include/wrenc_gpu.h: wrenc_gpu_download_complexity; the kernel is
wrenc_amd/csrc/dev_complexity.h) against tests/complexity_ref.py's numpy restatement, bit for bit: plane sums and the
CTU map, on content that reaches the arithmetic's extremes and at every seam of the kernel's layout (a wave is a strip
of 16 CTUs = 512 luma samples of one CTU row; a lane owns the luma blocks of rows 0 | 1, then 2 | 3 of that CTU row, then
one Cb | Cr pair, lanes 0..31 the upper and 32..63 the lower chroma block row), and the call's behaviour as an API."""
import numpy as np
import pytest

import complexity_ref as cr
from content import content

pytestmark = pytest.mark.gpu

# one CTU; two; 3 x 2 CTUs; 11 x 9 CTUs (a strip of 11, 9 CTU rows, 25 workgroups); 17 CTUs: one past a wave's strip
SIZES = [(32, 32), (64, 32), (96, 64), (352, 288), (544, 64)]
ESTATE, EINVAL = -5, -1


def _flat(w, h, v=93):
    return tuple(np.full(s, v, np.uint8) for s in ((h, w), (h // 2, w // 2), (h // 2, w // 2)))


def _noise(w, h, seed):
    rng = np.random.default_rng(seed)
    return tuple(rng.integers(0, 256, s, dtype=np.uint8) for s in ((h, w), (h // 2, w // 2), (h // 2, w // 2)))


def _figures(enc, pics):
    """The pictures through slots 0.. in ONE upload round and ONE call."""
    for k, p in enumerate(pics):
        enc.upload(k, *p)
    return enc.download_complexity(0, len(pics))


@pytest.mark.parametrize("w,h", SIZES)
def test_content_against_numpy(built, w, h):
    from wrenc_amd import gpu, synth
    pics = [_flat(w, h), _noise(w, h, 7), cr.checker1(w, h), cr.tiled(cr.bent_block(), w, h),
            synth.synth_textured_frame(w, h, 1), content("cclm", w, h, 2), content("extremes", w, h, 3)]
    enc = gpu.Encoder(w, h, qp=32, max_split_depth=2, n_slots=len(pics))
    got = _figures(enc, pics)
    enc.close()
    for g, p in zip(got, pics):
        cr.check(g, *p)
    # what the content was chosen for
    assert got[0]["satd"] == [0, 0, 0] and not got[0]["ctu_satd"].any()
    blocks = (w // 8) * (h // 8)
    assert got[2]["satd"] == [8160 * blocks, 8160 * blocks // 4, 8160 * blocks // 4]       # one coefficient of 32 * 255 per block
    assert got[3]["satd"] == [64260 * blocks, 64260 * blocks // 4, 64260 * blocks // 4]    # 63 coefficients of 4 * 255


def _spots(w, h):
    """(plane, block row, block column) of one noisy block: every plane's corners, and the layout's seams where the
    picture has them -- the luma rounds of a CTU row (block rows 1 | 2), CTU rows (3 | 4), the chroma lanes' two block rows
    (0 | 1) and CTU rows (1 | 2), CTUs (luma columns 3 | 4, chroma 1 | 2), strips (luma columns 63 | 64, chroma 31 | 32)."""
    out = set()
    for plane, bw, bh, rows, cols in ((0, w // 8, h // 8, (0, 1, 2, 3, 4), (0, 3, 4, 63, 64)),
                                     (1, w // 16, h // 16, (0, 1, 2), (0, 1, 2, 31, 32)),
                                     (2, w // 16, h // 16, (0, 1, 2), (0, 1, 2, 31, 32))):
        rr = sorted({min(r, bh - 1) for r in rows} | {bh - 1})
        cc = sorted({min(c, bw - 1) for c in cols} | {bw - 1})
        out |= {(plane, r, c) for r in rr for c in cc if (r in (0, bh - 1)) or (c in (0, bw - 1, 63, 64, 31, 32))}
    return sorted(out)


@pytest.mark.parametrize("w,h", [(32, 32), (96, 64), (544, 64)])
def test_one_noisy_block_lands_in_its_ctu(built, w, h):
    from wrenc_amd import gpu
    spots = _spots(w, h)
    rng = np.random.default_rng(w + h)
    pics = []
    for plane, r, c in spots:
        p = [a.copy() for a in _flat(w, h)]
        p[plane][8 * r:8 * r + 8, 8 * c:8 * c + 8] = rng.integers(0, 256, (8, 8), dtype=np.uint8)
        pics.append(tuple(p))
    enc = gpu.Encoder(w, h, qp=32, max_split_depth=2, n_slots=len(pics))
    got = _figures(enc, pics)
    enc.close()
    for (plane, r, c), g, p in zip(spots, got, pics):
        cr.check(g, *p)
        per_ctu = 4 if plane == 0 else 2
        hit = np.argwhere(g["ctu_satd"])
        assert hit.tolist() == [[r // per_ctu, c // per_ctu]], (plane, r, c, hit.tolist())
        assert g["satd"][plane] == int(g["ctu_satd"].sum()) > 0 and sum(g["satd"]) == g["satd"][plane]


def test_slots_calls_and_states(built):
    """The figures depend on the planes alone: not on the slot, on the call's size, or on whether the slot has been
    searched; a call made while a search of other slots is queued returns the right figures; and the error codes."""
    from wrenc_amd import gpu, synth
    w, h, n = 96, 64, 6
    pics = [synth.synth_textured_frame(w, h, k) for k in range(3)]
    refs = [cr.complexity(*p) for p in pics]
    enc = gpu.Encoder(w, h, qp=32, max_split_depth=2, n_slots=n)
    with pytest.raises(gpu.WrencGpuError) as e:            # nothing uploaded yet
        enc.download_complexity(0, 1)
    assert e.value.code == ESTATE
    for first, count in ((-1, 1), (0, 0), (n, 1), (n - 1, 2), (0, n + 1)):
        with pytest.raises(gpu.WrencGpuError) as e:
            enc.download_complexity(first, count)
        assert e.value.code == EINVAL, (first, count)
    enc.upload(0, *pics[0])
    enc.upload(1, *pics[1])
    enc.upload(n - 1, *pics[0])
    with pytest.raises(gpu.WrencGpuError) as e:            # slot 2 of the range is fresh
        enc.download_complexity(0, 3)
    assert e.value.code == ESTATE
    both = enc.download_complexity(0, 2)
    alone = [enc.download_complexity(0, 1)[0], enc.download_complexity(1, 1)[0], enc.download_complexity(n - 1, 1)[0]]
    for g, ref, p in zip(both + alone, [refs[0], refs[1], refs[0], refs[1], refs[0]], [pics[0], pics[1], pics[0], pics[1], pics[0]]):
        cr.check(g, *p, ref=ref)
    assert enc.download_complexity(0, 1, ctu_map=False)[0] == {"satd": refs[0]["satd"], "ctu_satd": None}
    # a search of slots 0, 1 is queued; slots 2.. are uploaded behind it and asked for at once
    enc.encode(0, 2)
    for k in (2, 3, 4):
        enc.upload(k, *pics[k - 2])
    queued = enc.download_complexity(2, 3)
    for g, ref, p in zip(queued, refs, pics):
        cr.check(g, *p, ref=ref)
    # ... and the searched slots still give what they gave before, with the search's results intact
    rec = [enc.download(k) for k in (0, 1)]
    after = enc.download_complexity(0, 2)
    for g, ref, p in zip(after, refs, pics):
        cr.check(g, *p, ref=ref)
    again = [enc.download(k) for k in (0, 1)]
    for a, b in zip(rec, again):
        assert all(np.array_equal(a[k], b[k]) for k in a)
    assert enc.final_pass_mismatches() == 0
    enc.close()
