"""An exact host model of the device sampler, for the tests.

Every device draw is a pure function of integers, so its exact answer can be
computed here.  The model is written from DESIGN 3.1 and the code it cites --
``make_perm_key`` (csrc/cf_kernels.hip), ``perm_rounds`` / ``permute``
(csrc/cf_device.h), ``sampler_args`` / ``cf_set_sampler_state``
(csrc/cf_engine.cpp), the slot key, ``draw_item`` and the group draw of
``prep_body`` (csrc/cf_kernels_impl.h) -- and imports nothing from the package.

It is deliberately literal:

* the scalar functions below use Python integers and are the definition;
* ``Model.sample`` evaluates the same definition over whole batches with numpy
  ``uint64`` (products wrap modulo 2^64 as the device's do; the 128-bit high
  multiply is written out in 32-bit halves), so that a 65,536-pair batch or a
  row that rejects 99.7 % of its candidates stays cheap;
* ``Model.sample_scalar`` evaluates it one pair at a time with the scalar
  functions and a Python ``set`` per user; tests/test_sampler_model.py holds
  the two together.

The model has NO inverse of the epoch bijection: a sorted batch is the sorted
forward images of its slots.  The device's inverse (64-bit and 32-bit forms),
its counting scatter and its radix sort all answer to the forward map alone.
"""
import numpy as np

M64 = (1 << 64) - 1
K_MAX_NEG = 64      # kMaxNeg, csrc/cf_kernels.h: the group draw's counters start there
K_MAX_GROUP = 16    # kMaxGroup
SLOT_MUL = 0xD1B54A32D192ED03


# ---------------------------------------------------------------------------
# the definition, in Python integers
# ---------------------------------------------------------------------------
def mix64(z):
    """SplitMix64 finaliser (cf_device.h)."""
    z = (z + 0x9E3779B97F4A7C15) & M64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M64
    return z ^ (z >> 31)


class PermKey(object):
    __slots__ = ("n", "bits", "mask", "shift", "k", "m")


def make_perm_key(n, seed, epoch):
    """The epoch bijection's key: the smallest width with 2^bits >= n (at
    least 1), shift = bits / 2 (at least 1), three xor keys below 2^bits and
    three odd 64-bit multipliers."""
    p = PermKey()
    p.n = n
    bits = 1
    while bits < 63 and (1 << bits) < n:
        bits += 1
    p.bits = bits
    p.mask = (1 << bits) - 1
    p.shift = bits // 2 if bits // 2 > 0 else 1
    h = mix64((seed ^ mix64((epoch + 0x5851F42D4C957F2D) & M64)) & M64)
    p.k, p.m = [], []
    for r in range(3):
        h = mix64((h + r) & M64)
        p.k.append(h & p.mask)
        p.m.append(mix64(h ^ 0xA0761D6478BD642F) | 1)
    return p


def perm_rounds(x, p):
    for r in range(3):
        x = (x ^ p.k[r]) & p.mask
        x = (x * p.m[r]) & p.mask
        x ^= x >> p.shift
    return x


def permute(slot, p):
    """Forward rounds on [0, 2^bits), cycle-walked back into [0, n)."""
    x = perm_rounds(slot, p)
    while x >= p.n:
        x = perm_rounds(x, p)
    return x


def rng_key(seed, epoch):
    return mix64(seed ^ mix64((epoch * 0x9E3779B97F4A7C15 + 0x2545F4914F6CDD1D) & M64))


def slot_key(rkey, slot):
    """The draw key of batch position ``slot`` = b B + p (in sorted batches the
    key belongs to the position, not to the pair that lands there)."""
    return mix64(rkey ^ ((slot * SLOT_MUL) & M64))


def draw_item(key, ctr, n_items):
    return (mix64((key + ctr) & M64) * n_items) >> 64


def negative(key, w, n_items, pos):
    """Negative w: the first attempt k = 0, 1, .. outside the user's set."""
    k = 0
    while True:
        j = draw_item(key, (w << 32) + k, n_items)
        if j not in pos:
            return j
        k += 1


def group_member(key, k, col):
    """Group user k: uniform over the item's column, with replacement."""
    h = mix64((key + ((K_MAX_NEG + k) << 32)) & M64)
    return col[(h * len(col)) >> 64]


# ---------------------------------------------------------------------------
# the same, over numpy uint64 arrays
# ---------------------------------------------------------------------------
def _u64(v):
    return np.uint64(v & M64)


def mix64_np(z):
    z = z + _u64(0x9E3779B97F4A7C15)
    z = (z ^ (z >> np.uint64(30))) * _u64(0xBF58476D1CE4E5B9)
    z = (z ^ (z >> np.uint64(27))) * _u64(0x94D049BB133111EB)
    return z ^ (z >> np.uint64(31))


def mulhi_np(h, n):
    """floor(h * n / 2^64) for uint64 h and 0 < n < 2^32 (elementwise):
    h = hi 2^32 + lo, so h n = hi n 2^32 + lo n with both products < 2^64."""
    n = np.asarray(n, dtype=np.uint64)
    assert (n < np.uint64(1 << 32)).all()
    s32 = np.uint64(32)
    hi, lo = h >> s32, h & np.uint64(0xFFFFFFFF)
    return (hi * n + ((lo * n) >> s32)) >> s32


def perm_rounds_np(x, p):
    mask, shift = _u64(p.mask), np.uint64(p.shift)
    for r in range(3):
        x = (x ^ _u64(p.k[r])) & mask
        x = (x * _u64(p.m[r])) & mask
        x = x ^ (x >> shift)
    return x


def permute_np(slots, p):
    x = perm_rounds_np(np.asarray(slots, dtype=np.uint64), p)
    out = np.nonzero(x >= np.uint64(p.n))[0]
    while out.size:
        x[out] = perm_rounds_np(x[out], p)
        out = out[x[out] >= np.uint64(p.n)]
    return x


def slot_key_np(rkey, slots):
    return mix64_np(_u64(rkey) ^ (np.asarray(slots, dtype=np.uint64) * _u64(SLOT_MUL)))


class Model(object):
    """The device sampler of one engine: ``sample(B)`` returns the batch
    ``cf_sample`` returns, ``state()`` what ``cf_get_sampler_state`` reports.

    ``gsize`` = 0: no group users (every model but GBPR)."""

    def __init__(self, indptr, indices, n_items, n_neg, gsize, seed, sorted=False):
        self.indptr = np.asarray(indptr, dtype=np.int64)
        self.indices = np.asarray(indices, dtype=np.int64)
        self.n_users = len(self.indptr) - 1
        self.n_items = int(n_items)
        self.nnz = int(self.indices.shape[0])
        assert self.indptr[0] == 0 and self.indptr[-1] == self.nnz and self.nnz >= 1
        assert 1 <= n_neg <= K_MAX_NEG and 0 <= gsize <= K_MAX_GROUP
        self.W, self.G = int(n_neg), int(gsize)
        self.seed = int(seed) & M64
        self.sorted = bool(sorted)
        # the pair array, in CSR (nonzero) order; empty rows contribute nothing
        self.pair_u = np.repeat(np.arange(self.n_users, dtype=np.int64), np.diff(self.indptr))
        self.pair_i = self.indices
        # Pos(u) as the ascending codes u n_items + i (rows are sorted, unique)
        self.pos_codes = self.pair_u * self.n_items + self.pair_i
        assert (np.diff(self.pos_codes) > 0).all(), "CSR rows must be sorted, unique"
        if self.G:   # item -> users, each column's users ascending
            o = np.argsort(self.pair_i, kind="stable")
            self.indices_t = self.pair_u[o]
            self.indptr_t = np.concatenate([[0], np.cumsum(np.bincount(self.pair_i, minlength=self.n_items))])
        self._sets = None
        self.epoch, self.batch, self.sampler_B = 0, 0, 0

    def fresh(self, n_neg=None, gsize=None, seed=None, sorted=None):
        """A model of another engine on the same graph (the graph's arrays are
        shared, the sampler position starts at (0, 0))."""
        import copy
        m = copy.copy(self)
        if gsize is not None and gsize and not self.G:
            raise ValueError("the group source was not built: construct the model with gsize > 0")
        m.W = self.W if n_neg is None else int(n_neg)
        m.G = self.G if gsize is None else int(gsize)
        m.seed = self.seed if seed is None else int(seed) & M64
        m.sorted = self.sorted if sorted is None else bool(sorted)
        assert 1 <= m.W <= K_MAX_NEG and 0 <= m.G <= K_MAX_GROUP
        m.epoch, m.batch, m.sampler_B = 0, 0, 0
        return m

    # ---- the state machine of sampler_args / cf_set_sampler_state -----------
    def state(self):
        return self.epoch, self.batch

    def set_state(self, epoch, batch):
        if epoch < 0 or batch < 0:
            raise ValueError("negative sampler state")
        self.epoch, self.batch = int(epoch), int(batch)

    def _advance(self, B):
        """Position for the next batch of B pairs: (epoch, first slot)."""
        if B < 1 or B > self.nnz:
            raise ValueError("batch size exceeds the number of interactions")
        if self.sampler_B != B:
            if self.sampler_B != 0 and self.batch != 0:   # a new B inside an epoch: the next epoch's start
                self.epoch += 1
                self.batch = 0
            self.sampler_B = B
        per_epoch = self.nnz // B
        if self.batch >= per_epoch:
            self.epoch += 1
            self.batch = 0
        at = (self.epoch, self.batch * B)
        self.batch += 1
        return at

    # ---- one batch ----------------------------------------------------------
    def batch_pairs(self, epoch, slot0, B, n_batches=1):
        """Pair indices of the slots [slot0, slot0 + n_batches B) of ``epoch``,
        in the order the draw visits them (sorted: each batch ascending)."""
        p = make_perm_key(self.nnz, self.seed, epoch)
        q = permute_np(np.arange(slot0, slot0 + n_batches * B, dtype=np.uint64), p).astype(np.int64)
        return np.sort(q.reshape(n_batches, B), axis=1).ravel() if self.sorted else q

    def sample(self, B):
        epoch, slot0 = self._advance(B)
        return self.draw(epoch, slot0, B)

    def sample_many(self, B, n):
        """n consecutive ``sample(B)`` calls as a list of batches; the batches
        of one epoch are drawn in one pass."""
        at = [self._advance(B) for _ in range(n)]
        out, s = [], 0
        while s < n:
            t = s + 1
            while t < n and at[t] == (at[s][0], at[t - 1][1] + B):
                t += 1
            pairs, negs, groups = self.draw(at[s][0], at[s][1], B, t - s)
            for b in range(t - s):
                r = slice(b * B, (b + 1) * B)
                out.append((pairs[r], negs[r], None if groups is None else groups[r]))
            s = t
        return out

    def draw(self, epoch, slot0, B, n_batches=1):
        """The batch at the slots [slot0, slot0 + B) of ``epoch`` (n_batches
        > 1: that many consecutive batches of one epoch, concatenated)."""
        assert slot0 + n_batches * B <= self.nnz
        q = self.batch_pairs(epoch, slot0, B, n_batches)
        B = n_batches * B
        u, i = self.pair_u[q], self.pair_i[q]
        key = slot_key_np(rng_key(self.seed, epoch), np.arange(slot0, slot0 + B, dtype=np.uint64))
        W, ni = self.W, self.n_items
        # negative w of position p: attempts k = 0, 1, .. until one is outside Pos(u)
        negs = np.empty(B * W, dtype=np.int64)
        kk = np.repeat(key, W)
        uu = np.repeat(u, W)
        ctr = np.tile(np.arange(W, dtype=np.uint64) << np.uint64(32), B)
        todo = np.arange(B * W)
        A = 1   # attempts looked at per pass: the first alone, then the next 32 of those still open
        while todo.size:
            k = np.arange(A, dtype=np.uint64)
            j = mulhi_np(mix64_np((kk[todo] + ctr[todo])[:, None] + k), ni).astype(np.int64)
            code = uu[todo][:, None] * ni + j
            at = np.searchsorted(self.pos_codes, code)
            hit = self.pos_codes[np.minimum(at, self.nnz - 1)] == code
            first = np.argmin(hit, axis=1)              # the first attempt outside Pos(u), if any is
            done = ~hit[np.arange(todo.size), first]
            negs[todo[done]] = j[done, first[done]]
            todo = todo[~done]
            ctr[todo] += np.uint64(A)
            A = 32
        groups = None
        if self.G:
            cb, ce = self.indptr_t[i], self.indptr_t[i + 1]
            groups = np.empty((B, self.G), dtype=np.int64)
            for k in range(self.G):
                h = mix64_np(key + _u64((K_MAX_NEG + k) << 32))
                groups[:, k] = self.indices_t[cb + mulhi_np(h, ce - cb).astype(np.int64)]
        pairs = np.stack([u, i], axis=1).astype(np.int32)
        return pairs, negs.reshape(B, W).astype(np.int32), None if groups is None else groups.astype(np.int32)

    # ---- the same batch, one pair at a time, in Python integers --------------
    def sample_scalar(self, B):
        epoch, slot0 = self._advance(B)
        return self.draw_scalar(epoch, slot0, B)

    def draw_scalar(self, epoch, slot0, B):
        if self._sets is None:
            self._sets = [set(self.indices[self.indptr[u]:self.indptr[u + 1]].tolist())
                          for u in range(self.n_users)]
        p = make_perm_key(self.nnz, self.seed, epoch)
        q = [permute(s, p) for s in range(slot0, slot0 + B)]
        if self.sorted:
            q = sorted(q)
        rkey = rng_key(self.seed, epoch)
        pairs, negs, groups = [], [], []
        for pos, qq in enumerate(q):
            u, i = int(self.pair_u[qq]), int(self.pair_i[qq])
            key = slot_key(rkey, slot0 + pos)
            pairs.append((u, i))
            negs.append([negative(key, w, self.n_items, self._sets[u]) for w in range(self.W)])
            if self.G:
                col = self.indices_t[self.indptr_t[i]:self.indptr_t[i + 1]]
                groups.append([int(group_member(key, k, col)) for k in range(self.G)])
        return (np.array(pairs, np.int32).reshape(B, 2), np.array(negs, np.int32).reshape(B, self.W),
                np.array(groups, np.int32).reshape(B, self.G) if self.G else None)


def csr_from_rows(rows, n_users=None):
    """(indptr int64, indices int32) of a list of per-user item lists (each
    sorted here); users past the list have empty rows."""
    n_users = len(rows) if n_users is None else n_users
    lens = [len(r) for r in rows] + [0] * (n_users - len(rows))
    indptr = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    indices = (np.concatenate([np.sort(np.asarray(r, dtype=np.int32)) for r in rows if len(r)])
               if indptr[-1] else np.zeros(0, np.int32))
    return indptr, indices.astype(np.int32)
