"""CPU: the work partition of WorkQueue (csrc/sor_grid_params.h: wq_init, wq_next) restated in Python.

Group y = blockIdx % 8 owns the items [n y / 8, n (y + 1) / 8).  Its waves stride through a static share of that range
(WQ_STATIC_PCT % of it, rounded down to full rounds of the group's waves) and take the rest -- the tail -- one by one from the
group's counter.  Nothing crosses a group boundary.  Claims checked here, for every interleaving of the waves' requests that
is tried: every item is handed out exactly once; an item of the static share goes to the wave that strides over it and an item
of the tail to some wave of the same group; every counter ends at its tail length + one failed request per wave of the group."""
import numpy as np
import pytest

WAVES_PER_BLOCK = 4
STATIC_PCT = 50     # WQ_STATIC_PCT
ITEMS = [0, 1, 7, 8, 9, 5119, 5120, 5121, 168414]
GRIDS = [1280, 1536]   # workgroups: 256 CUs x 5 (knn_brick at k = 16) and x 6 (knn_ring_fast)


def wq_range(n, y, grid, wpb=WAVES_PER_BLOCK):
    """-> lo, hi, stride, static_end of group y: the arithmetic of wq_init in csrc/sor_grid_params.h"""
    lo, hi = n * y // 8, n * (y + 1) // 8
    stride = ((grid + 7 - y) // 8) * wpb
    rounds = ((hi - lo) * STATIC_PCT // 100) // stride
    return lo, hi, stride, lo + rounds * stride


class Wave:
    def __init__(self, n, block, wave, grid):
        self.y = block & 7
        lo, hi, stride, static_end = wq_range(n, self.y, grid)
        self.next = lo + (block >> 3) * WAVES_PER_BLOCK + wave
        self.static_end, self.end, self.stride = static_end, hi, stride
        self.took = [0, 0]   # static share, tail

    def take(self, ctr):
        """wq_next: the next item or -1.  ctr: the eight counters"""
        if self.next < self.static_end:
            b = self.next
            self.next += self.stride
            self.took[0] += 1
            return b
        if self.static_end >= self.end:
            return -1
        t = ctr[self.y]
        ctr[self.y] += 1
        b = self.static_end + t
        if b < self.end:
            self.took[1] += 1
            return b
        return -1


def run(n, grid, order_seed):
    """every wave asks until it is told -1; order_seed None: wave after wave, else a random interleaving of the requests"""
    waves = [Wave(n, b, w, grid) for b in range(grid) for w in range(WAVES_PER_BLOCK)]
    ctr = [0] * 8
    owner = np.full(n, -1, np.int64)
    handed = np.zeros(n, np.int64)

    def ask(i):
        b = waves[i].take(ctr)
        if b >= 0:
            assert 0 <= b < n
            handed[b] += 1
            owner[b] = i
        return b >= 0

    if order_seed is None:
        for i in range(len(waves)):
            while ask(i):
                pass
    else:
        rng = np.random.default_rng(order_seed)
        live = list(range(len(waves)))
        while live:
            # a burst of requests in random order; slow waves (a random third: the youngest wave of a SIMD gets the issue
            # slots its elders leave) ask less often
            slow = rng.random(len(live)) < 0.33
            nxt = []
            for j in rng.permutation(len(live)):
                i = live[j]
                if slow[j] and rng.random() < 0.8:
                    nxt.append(i)
                    continue
                if ask(i):
                    nxt.append(i)
            live = nxt
    return waves, ctr, handed, owner


@pytest.mark.parametrize("grid", GRIDS)
@pytest.mark.parametrize("n", ITEMS)
def test_every_item_is_handed_out_exactly_once(n, grid):
    for seed in (None, 1, 2, 3):
        waves, ctr, handed, owner = run(n, grid, seed)
        assert np.all(handed == 1), (n, grid, seed, np.nonzero(handed != 1)[0][:8])
        home = np.array([w.y for w in waves])
        for y in range(8):
            lo, hi, stride, static_end = wq_range(n, y, grid)
            tail = hi - static_end
            assert np.all(home[owner[lo:hi]] == y)   # nothing crosses a group boundary
            st = np.arange(lo, static_end)           # static share: the wave that strides over it and no other
            if len(st):
                wl = (owner[st] // WAVES_PER_BLOCK >> 3) * WAVES_PER_BLOCK + owner[st] % WAVES_PER_BLOCK
                assert np.all((st - lo) % stride == wl)
            # the counter: one request per item of the tail and one failed request per wave of the group
            assert ctr[y] == (tail + stride if tail > 0 else 0), (y, tail, ctr[y])
        took = np.array([w.took for w in waves]).sum(axis=0)
        assert took.sum() == n


@pytest.mark.parametrize("grid", GRIDS)
@pytest.mark.parametrize("n", ITEMS)
def test_the_static_shares_and_tails_tile_the_items(n, grid):
    """the ranges of the eight groups tile [0, n); a static share is full rounds of the group's waves and as close below
    WQ_STATIC_PCT % of the range as full rounds allow; 1280 and 1536 are multiples of 8: every group has grid / 8 blocks"""
    edge = 0
    for y in range(8):
        lo, hi, stride, static_end = wq_range(n, y, grid)
        assert lo == edge and hi >= lo
        edge = hi
        assert stride == (grid // 8) * WAVES_PER_BLOCK
        assert lo <= static_end <= hi and (static_end - lo) % stride == 0
        assert static_end - lo <= (hi - lo) * STATIC_PCT // 100 < static_end - lo + stride
    assert edge == n


def test_the_stride_follows_the_grid_remainder():
    """a grid that is no multiple of 8: the first grid % 8 groups have one block more"""
    n, grid = 100000, 1283
    for y in range(8):
        lo, hi, stride, static_end = wq_range(n, y, grid)
        assert stride == (160 + (1 if y < 3 else 0)) * WAVES_PER_BLOCK
    waves, ctr, handed, owner = run(n, grid, 7)
    assert np.all(handed == 1)


def test_a_starved_wave_keeps_only_its_static_share():
    """why the static share is no larger: a wave that gets no issue slots until its elders have left still
    owns its static rounds -- nobody else can take them -- but none of the tail"""
    n, grid = 168414, 1280
    waves = [Wave(n, b, w, grid) for b in range(grid) for w in range(WAVES_PER_BLOCK)]
    ctr = [0] * 8
    starved = [i for i in range(len(waves)) if (i // WAVES_PER_BLOCK) % 5 == 4]
    fed = [i for i in range(len(waves)) if (i // WAVES_PER_BLOCK) % 5 != 4]
    for i in fed:
        while waves[i].take(ctr) >= 0:
            pass
    for i in starved:
        k = 0
        while waves[i].take(ctr) >= 0:
            k += 1
        lo, hi, stride, static_end = wq_range(n, waves[i].y, grid)
        assert k == (static_end - lo) // stride and waves[i].took[1] == 0
