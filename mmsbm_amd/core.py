"""Thin Python handle over the resident C-ABI context (include/mmsbm_hip.h, "level 2").

One ``HipEM`` = one GPU + one encoded training set.  Parameters stay on the device
between calls; the EM loop of src/mmsbm.py:243-250 runs there without host round trips.
"""
from __future__ import annotations

import ctypes as C
import hashlib

import numpy as np

from . import _lib


def _i32(a):
    return np.ascontiguousarray(a, dtype=np.int32)


def _f64(a):
    return np.ascontiguousarray(a, dtype=np.float64)


def _p(a, ctype):
    return a.ctypes.data_as(C.POINTER(ctype))


def _p_or_null(a, ctype):
    """_p for an optional array: None is the null pointer."""
    return None if a is None else _p(a, ctype)


def _csr(lists, rows, name, noun):
    """(offsets int64, values int32) of a CSR argument ``lists`` = (offsets, values) over ``rows`` rows, its ``name``
    and the ``noun`` of its values in the shape and end checks; (None, None) for None, an optional list left out."""
    if lists is None:
        return None, None
    offsets, values = lists
    off = np.ascontiguousarray(offsets, dtype=np.int64)
    val = _i32(values)
    if off.shape != (rows + 1,):
        raise ValueError(f"{name} have shape {off.shape}, expected ({rows + 1},)")
    if off[-1] != len(val):
        raise ValueError(f"{name} end at {int(off[-1])}, {noun} holds {len(val)}")
    return off, val


def _row_csr(lists, rows, name, noun):
    """_csr of an optional list as the C ABI takes it: (offsets pointer, values pointer); null, null for None."""
    off, val = _csr(lists, rows, name, noun)
    return _p_or_null(off, C.c_int64), _p_or_null(val, C.c_int32)


def _subset(candidates):
    """(n_cand, cand_items) of an optional candidate subset; (0, null) for None, the whole catalogue."""
    cand = None if candidates is None else _i32(candidates)
    return 0 if cand is None else len(cand), _p_or_null(cand, C.c_int32)


def _user_set(users, when_none):
    """(n_users, users) of an optional user set; (when_none, null) for None, every training user."""
    u = None if users is None else _i32(users)
    return when_none if u is None else len(u), _p_or_null(u, C.c_int32)


def _slot_blocks(values, name, expected, width, added):
    """``values`` as float64 (S, rows, width), one block per slot a session holds ``added`` of; ``expected``: how the
    refusal of another shape ends."""
    a = _f64(values)
    if a.ndim != 3 or a.shape[2] != width:
        raise ValueError(f"{name} has shape {a.shape}, {expected}")
    if a.shape[0] != added:
        raise ValueError(f"{name} holds {a.shape[0]} blocks, the session {added} added slots")
    return a


def _fetch_i32(symbol, *head):
    """The int32 array of count-then-fill entry ``symbol(*head, out, capacity, count)``: asked for its length, then, if
    it has any, filled."""
    cnt = C.c_int64(0)
    _lib.call(symbol, *head, None, 0, C.byref(cnt))
    arr = np.empty(cnt.value, dtype=np.int32)
    if cnt.value:
        _lib.call(symbol, *head, _p(arr, C.c_int32), arr.size, C.byref(cnt))
    return arr


def normalize_with_self(p):
    """p[k,l,:] /= sum_r p[k,l,r]; zero rows stay zero (src/expectation_maximization.py:152-155).
    Host-side, used for the random initialisation only."""
    flat = p.reshape(-1, p.shape[2])
    tot = flat.sum(axis=1)
    return (flat / np.where(tot == 0, 1, tot)[:, None]).reshape(p.shape)


def pcg64_words(bit_generator):
    """{state_hi, state_lo, inc_hi, inc_lo} of a numpy PCG64, as the C ABI takes them."""
    st = bit_generator.state["state"]
    mask = (1 << 64) - 1
    return (C.c_uint64 * 4)(st["state"] >> 64, st["state"] & mask, st["inc"] >> 64, st["inc"] & mask)


def pcg64_doubles(seed, offset, n):
    """n doubles of default_rng(seed)'s stream starting `offset` draws in, from the library's own
    generator (host code; no GPU needed)."""
    out = np.empty(int(n), dtype=np.float64)
    _lib.call("mmsbm_hip_pcg64_doubles", pcg64_words(np.random.PCG64(seed)), int(offset), int(n),
              _p(out, C.c_double))
    return out


def split_triples(data):
    """(N,3) integer array (any int dtype, any strides) -> three contiguous int32 columns."""
    d = np.asarray(data)
    if d.ndim != 2 or d.shape[1] < 3:
        raise ValueError("data must have shape (N, 3): [user_idx, item_idx, rating_idx]")
    if d.shape[0] and not np.issubdtype(d.dtype, np.integer):
        raise TypeError("data must hold integer ids")
    if d.size and (d.min() < 0 or d.max() >= 2**31):
        raise ValueError("ids must be in [0, 2^31)")
    return _i32(d[:, 0]), _i32(d[:, 1]), _i32(d[:, 2])


try:  # 128-bit XXH3: ~10 GB/s (about 2.4 ms per million (N,3) int64 rows); blake2b does ~1 GB/s
    from xxhash import xxh3_128 as _digest128
    DIGEST = "xxh3_128"
except ImportError:  # pragma: no cover - depends on the environment
    DIGEST = "blake2b"
    _warned = []

    def _digest128(buf):
        # `xxhash` is an optional dependency (requirements.txt lists it): without it the digest of a level-1 call is
        # ten times slower and no longer hides behind the GPU work (level 1) -- say so, once
        if not _warned:
            _warned.append(True)
            import warnings
            warnings.warn("mmsbm_amd: the `xxhash` module is not installed; the training-set digest of the level-1 "
                          "backend (kernels_hip) falls back to blake2b, about ten times slower per call",
                          RuntimeWarning, stacklevel=3)
        return hashlib.blake2b(buf, digest_size=16)


def data_key(data):
    """Exact identity of a set of encoded triples: (shape, dtype, 128-bit digest over EVERY byte of
    the first three columns).  Two training sets that differ anywhere -- two rows swapped, two
    ratings exchanged, a re-shuffled fold -- get different keys (the level-1 cache of kernels_hip
    and ``MMSBM.compute_likelihood`` rely on that).  Pure host code."""
    d = np.asarray(data)
    if d.ndim != 2 or d.shape[1] < 3:
        raise ValueError("data must have shape (N, 3): [user_idx, item_idx, rating_idx]")
    d = np.ascontiguousarray(d[:, :3])
    return (d.shape, d.dtype.str, _digest128(memoryview(d).cast("B")).hexdigest())


LAYOUT_NAMES = ["pair_off", "pair_user", "pair_item", "rating_off", "user_off", "user_pair",
                "item_off", "item_pairs", "item_deg", "chunk_off", "chunks", "mv_chunks",
                "pair_items", "user_items", "pair_splits", "user_splits"]       # mmsbm_hip_layout_array: which = position
INDEX_ONLY_NAMES = ["item_grid", "lik_units", "mv_chunk_off"]                   # mmsbm_hip_index_array: 16, 17, 18
RECORD_NAMES = frozenset(LAYOUT_NAMES[10:] + ["lik_units"])                     # arrays of 4-int records


class HipEM:
    """Device-resident EM state for one (GPU, training set, K, L)."""

    def __init__(self, data, k_groups, l_groups, n_users=None, n_items=None, n_ratings=None,
                 device=0, swap_sides=-1, slots=1):
        u, i, r = split_triples(data)
        n = len(u)
        self.n_obs = n
        self.n_users = int(n_users) if n_users is not None else (int(u.max()) + 1 if n else 1)
        self.n_items = int(n_items) if n_items is not None else (int(i.max()) + 1 if n else 1)
        self.n_ratings = int(n_ratings) if n_ratings is not None else (int(r.max()) + 1 if n else 1)
        self.k, self.l = int(k_groups), int(l_groups)
        self.device = int(device)
        self._h = C.c_void_p()
        _lib.call("mmsbm_hip_create", self.device, n, self.n_users, self.n_items, self.n_ratings,
                  self.k, self.l, _p(u, C.c_int32), _p(i, C.c_int32), _p(r, C.c_int32),
                  int(swap_sides), C.byref(self._h))
        dims = (C.c_int64 * 8)()
        _lib.call("mmsbm_hip_dims", self._h, dims)
        self.n_pairs, self.swapped = int(dims[6]), bool(dims[7])
        self.slots = 1
        self._rc_added = 0
        self._ho_rows = 0
        if int(slots) != 1:
            self.set_slots(slots)

    def suggested_slots(self, most=8):
        """How many restarts to advance together as slots of one launch.  Slots share the index stream and
        turn a gathered row into whole cache lines, which pays while the slot-interleaved gathered tables
        (rows x K x 8 bytes x slots) stay below roughly 700 MB; beyond that the gathers get slower than the
        sharing saves.  Measured per restart-iteration, 1 / 4 / 8 slots: 1M ratings K=20 98 / 77 / 75 us,
        10M x 1M users K=20 1,046 / 838 / 919, 4M x 400k K=50 905 / 878 / 886, 10M x 1M K=50 (BASELINE
        config 5) 2,213 / 2,469 / 2,394 -- there the restarts run one after the other."""
        rows = max(self.n_items if self.swapped else self.n_users, self.n_pairs)
        groups = self.l if self.swapped else self.k
        table = rows * 8 * (-(-groups // 4) * 4)
        s = max(1, int(most))
        while s > 1 and s * table > 700 * 2 ** 20:
            s //= 2
        return s

    # -- lifetime ------------------------------------------------------------------------
    def close(self):
        if getattr(self, "_h", None) is not None and self._h.value:
            _lib.call("mmsbm_hip_destroy", self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    # -- restart slots -------------------------------------------------------------------
    def set_slots(self, n_slots):
        """Hold ``n_slots`` independent restarts (parameter sets) over the same triples;
        ``iterate`` advances all of them with one set of launches, everything else acts on
        the selected slot.  Drops all parameters and selects slot 0.  If the device runs out of
        memory the library falls back to ONE slot and this raises; ``slots`` always reports
        what the context really holds."""
        try:
            _lib.call("mmsbm_hip_set_slots", self._h, int(n_slots))
        finally:
            n = C.c_int(1)
            _lib.call("mmsbm_hip_slots", self._h, C.byref(n), None, None)
            self.slots = int(n.value)

    def select(self, slot):
        _lib.call("mmsbm_hip_select_slot", self._h, int(slot))
        return self

    @property
    def selected(self):
        s = C.c_int(0)
        _lib.call("mmsbm_hip_slots", self._h, None, C.byref(s), None)
        return int(s.value)

    @property
    def bytes_per_slot(self):
        """Device memory one restart slot occupies (parameters, A/C/T tables, slabs)."""
        b = C.c_int64(0)
        _lib.call("mmsbm_hip_slots", self._h, None, None, C.byref(b))
        return int(b.value)

    def max_slots(self, fraction=0.5, sharers=1):
        """How many slots fit in `fraction` of the memory that is FREE on the device right now
        (hipMemGetInfo: other contexts and processes already count) plus what this context's own
        slots hold, divided among `sharers` workers that size their batches at the same time
        (contexts_per_device, cv_fit lanes that repeat a GPU).  At least 1."""
        free = C.c_int64(0)
        _lib.call("mmsbm_hip_device_mem", self.device, C.byref(free), None)
        per = max(self.bytes_per_slot, 1)
        mine = per * self.slots  # re-used by the next set_slots
        return max(1, int(fraction * (free.value / max(int(sharers), 1) + mine)) // per)

    # -- parameters ----------------------------------------------------------------------
    def _shapes(self):
        return ((self.n_users, self.k), (self.n_items, self.l), (self.k, self.l, self.n_ratings))

    def set_params(self, theta, eta, pr):
        theta, eta, pr = _f64(theta), _f64(eta), _f64(pr)
        for arr, shp, nm in zip((theta, eta, pr), self._shapes(), ("theta", "eta", "pr")):
            if arr.shape != shp:
                raise ValueError(f"{nm} has shape {arr.shape}, expected {shp}")
        _lib.call("mmsbm_hip_set_params", self._h, _p(theta, C.c_double), _p(eta, C.c_double),
                  _p(pr, C.c_double))

    def init_params(self, seed):
        """The reference's random start (src/mmsbm.py:224-233) generated on the device:
        theta0 and eta0 are drawn there from ``default_rng(seed)``'s PCG64 stream (bit-identical
        to numpy), only the small p0 is drawn on the host.  Returns p0."""
        bg = np.random.PCG64(seed)
        words = pcg64_words(bg)
        bg.advance(self.n_users * self.k + self.n_items * self.l)
        pr = normalize_with_self(np.random.Generator(bg).random((self.k, self.l, self.n_ratings)))
        _lib.call("mmsbm_hip_init_params", self._h, words, _p(pr, C.c_double))
        return pr

    def get_params(self):
        theta, eta, pr = (np.empty(s, dtype=np.float64) for s in self._shapes())
        _lib.call("mmsbm_hip_get_params", self._h, _p(theta, C.c_double), _p(eta, C.c_double),
                  _p(pr, C.c_double))
        return theta, eta, pr

    def result(self):
        """(likelihood, theta, eta, pr) of the selected slot: what likelihood() and get_params() return, the
        download overlapped with the likelihood kernels."""
        theta, eta, pr = (np.empty(s, dtype=np.float64) for s in self._shapes())
        out = C.c_double(0.0)
        _lib.call("mmsbm_hip_result", self._h, _p(theta, C.c_double), _p(eta, C.c_double), _p(pr, C.c_double),
                  C.byref(out))
        return np.float64(out.value), theta, eta, pr

    def degrees(self):
        d_u = np.empty(self.n_users, dtype=np.int64)
        d_i = np.empty(self.n_items, dtype=np.int64)
        _lib.call("mmsbm_hip_degrees", self._h, _p(d_u, C.c_int64), _p(d_i, C.c_int64))
        return d_u, d_i

    # -- the hot path ----------------------------------------------------------------------
    def iterate(self, n_iters, sync=True):
        _lib.call("mmsbm_hip_em_iterate", self._h, int(n_iters))
        if sync:
            self.synchronize()

    def synchronize(self):
        _lib.call("mmsbm_hip_synchronize", self._h)

    def update_coefficients(self):
        n_theta, n_eta, n_pr = (np.empty(s, dtype=np.float64) for s in self._shapes())
        _lib.call("mmsbm_hip_update_coefficients", self._h, _p(n_theta, C.c_double),
                  _p(n_eta, C.c_double), _p(n_pr, C.c_double))
        return n_theta, n_eta, n_pr

    def likelihood(self):
        out = C.c_double(0.0)
        _lib.call("mmsbm_hip_likelihood", self._h, C.byref(out))
        return np.float64(out.value)

    def compute_omegas(self):
        out = np.empty((self.n_obs, self.k, self.l), dtype=np.float64)
        _lib.call("mmsbm_hip_compute_omegas", self._h, _p(out, C.c_double), out.size)
        return out

    def prod_dist(self, pairs):
        d = np.asarray(pairs)
        if d.ndim != 2 or d.shape[1] < 2:
            raise ValueError("pairs must have shape (M, >=2): [user_idx, item_idx, ...]")
        u, i = _i32(d[:, 0]), _i32(d[:, 1])
        out = np.empty((len(u), self.n_ratings), dtype=np.float64)
        _lib.call("mmsbm_hip_prod_dist", self._h, len(u), _p(u, C.c_int32), _p(i, C.c_int32),
                  _p(out, C.c_double))
        return out

    # -- predict / score on the device (src/mmsbm.py:297-315, 488-539) ----------------------
    STAT_NAMES = ("rows", "true", "almost", "s2", "true_pond", "s2pond")

    @staticmethod
    def final_stats(raw):
        """The reference's five scores (src/mmsbm.py:530-539) from the six device sums."""
        n = raw[0]
        with np.errstate(divide="ignore", invalid="ignore"):
            return {"accuracy": np.float64(raw[1]) / n, "one_off_accuracy": np.float64(raw[2]) / n,
                    "mae": 1 - np.float64(raw[4]) / n, "s2": np.int64(raw[3]), "s2pond": np.float64(raw[5])}

    def predict_begin(self, test, rating_weights):
        """Open a scoring session over (M,3) test triples [user, item, true rating index]."""
        u, i, r = split_triples(test)
        w = _f64(rating_weights)
        if w.shape != (self.n_ratings,):
            raise ValueError(f"rating_weights has shape {w.shape}, expected ({self.n_ratings},)")
        self._ps_rows = len(u)
        _lib.call("mmsbm_hip_predict_begin", self._h, len(u), _p(u, C.c_int32), _p(i, C.c_int32),
                  _p(r, C.c_int32), _p(w, C.c_double))

    def predict_add(self):
        """Add the selected slot's rating distribution to the session; its six raw sums."""
        st = np.zeros(6, dtype=np.float64)
        _lib.call("mmsbm_hip_predict_add", self._h, _p(st, C.c_double))
        return st

    def predict_finish(self, want_matrix=True):
        """(mean distribution (M,R) or None, six raw sums of the mean); closes the session."""
        st = np.zeros(6, dtype=np.float64)
        out = np.empty((self._ps_rows, self.n_ratings), dtype=np.float64) if want_matrix else None
        _lib.call("mmsbm_hip_predict_finish", self._h,
                  _p(out, C.c_double) if want_matrix else None, _p(st, C.c_double))
        return out, st

    # -- top-N recommendation on the device (include/mmsbm_hip.h: mmsbm_hip_recommend_*) --------------
    MAX_RECOMMEND = 1024

    def recommend_begin(self, rating_weights, exclude_seen=True):
        """Open a recommend session: score = sum_r w_r P(r | u, i), averaged over the slots added to it."""
        w = _f64(rating_weights)
        if w.shape != (self.n_ratings,):
            raise ValueError(f"rating_weights has shape {w.shape}, expected ({self.n_ratings},)")
        _lib.call("mmsbm_hip_recommend_begin", self._h, _p(w, C.c_double), int(bool(exclude_seen)))
        self._rc_added = 0

    def recommend_add(self):
        """Fold the selected slot's current parameters into the session (the slot is left unchanged)."""
        _lib.call("mmsbm_hip_recommend_add", self._h)
        self._rc_added += 1

    @staticmethod
    def _query_out(m, n):
        """Empty (items, scores, counts) of a query of m users."""
        return (np.empty((m, max(n, 0)), dtype=np.int32), np.empty((m, max(n, 0)), dtype=np.float64),
                np.empty(m, dtype=np.int32))

    def _top_n(self, symbol, ids, n):
        """(ids (M,n) int32, values (M,n), counts (M,)) of top-N entry ``symbol`` for the M encoded ids ``ids``."""
        q, n = _i32(ids), int(n)
        out, values, counts = self._query_out(len(q), n)
        _lib.call(symbol, self._h, len(q), _p(q, C.c_int32), n, _p(out, C.c_int32), _p(values, C.c_double),
                  _p(counts, C.c_int32))
        return out, values, counts

    def recommend_query(self, users, n):
        """(items (M,n) int32 padded with -1, scores (M,n) padded with -inf, counts (M,)) for encoded user ids."""
        return self._top_n("mmsbm_hip_recommend_query", users, n)

    def _theta_rows(self, theta, added):
        """(theta as float64 (S, M, K), M) of caller-given users for a session that holds ``added`` slots."""
        t = _slot_blocks(theta, "theta", f"expected (slots, users, {self.k})", self.k, added)
        return t, t.shape[1]

    def _theta_query(self, t, m, seen, candidates):
        """The leading arguments of a query over the ``m`` theta rows ``t``: handle, rows, seen lists, candidate subset
        (left out for None where the entry has none)."""
        return (self._h, m, _p(t, C.c_double), *_row_csr(seen, m, "seen offsets", "items"), *_subset(candidates))

    def recommend_query_theta(self, theta, n, seen=None, candidates=None):
        """recommend_query for caller-given users: theta (S, M, K), one (M, K) block per added slot in add order.
        seen: None (nothing excluded) or (offsets (M+1,) int64, items int32): user b leaves out
        items[offsets[b]:offsets[b + 1]].  candidates: None (the whole catalogue) or ascending, distinct item ids of
        the session's catalogue, as in recommend_query_within."""
        (t, m), n = self._theta_rows(theta, self._rc_added), int(n)
        head = self._theta_query(t, m, seen, candidates)
        items, scores, counts = self._query_out(m, n)
        tail = (n, _p(items, C.c_int32), _p(scores, C.c_double), _p(counts, C.c_int32))
        if candidates is None:
            _lib.call("mmsbm_hip_recommend_query_theta", *head[:-2], *tail)
        else:
            _lib.call("mmsbm_hip_recommend_query_theta_within", *head, *tail)
        return items, scores, counts

    def _user_query(self, u, candidates, exclude):
        """The leading arguments of a query over the encoded users ``u``: handle, users, candidate subset, exclusions."""
        return (self._h, len(u), _p(u, C.c_int32), *_subset(candidates),
                *_row_csr(exclude, len(u), "exclude offsets", "items"))

    def recommend_query_within(self, users, n, candidates=None, exclude=None):
        """recommend_query within a part of the catalogue: the n best of ``candidates`` (ascending, distinct item ids
        of the session's catalogue; None: all of it) for each encoded user id, without what recommend_query leaves out
        and without ``exclude``: None or (offsets (M+1,) int64, items int32), request row b also leaves out
        items[offsets[b]:offsets[b + 1]] (any order; a user asked twice may carry two lists).  Scores and order are
        recommend_query's: the answer is its row for n = all items, filtered and cut to n."""
        u, n = _i32(users), int(n)
        items, scores, counts = self._query_out(len(u), n)
        _lib.call("mmsbm_hip_recommend_query_within", *self._user_query(u, candidates, exclude), n,
                  _p(items, C.c_int32), _p(scores, C.c_double), _p(counts, C.c_int32))
        return items, scores, counts

    @staticmethod
    def _pcg64_state(state):
        """The four state words of the C ABI: ``pcg64_words``' array as it is, or those of a numpy PCG64 bit
        generator (left where it stands); None: a null pointer, which the library refuses."""
        return pcg64_words(state) if hasattr(state, "state") else state

    def recommend_query_explore(self, users, n, temperature, state, candidates=None, exclude=None):
        """recommend_query_within drawn at random: each row's list is sampled without replacement from the
        Plackett-Luce distribution over the row's candidates with utilities score / ``temperature`` -- the n largest
        of score + temperature * g(user, item), g the Gumbel noise of draw number (user << 32 | item) of the PCG64
        stream ``state`` (``pcg64_words``' four words, or the bit generator itself) -- and every position comes with
        the probability the policy had of showing it there.  Returns (items, scores, propensity (M,n) padded with 0,
        counts); scores are recommend_query's bits of the listed items, not the perturbed keys."""
        u, n = _i32(users), int(n)
        items, scores, counts = self._query_out(len(u), n)
        prop = np.empty((len(u), max(n, 0)), dtype=np.float64)
        _lib.call("mmsbm_hip_recommend_query_explore", *self._user_query(u, candidates, exclude), n, float(temperature),
                  self._pcg64_state(state), _p(items, C.c_int32), _p(scores, C.c_double), _p(prop, C.c_double),
                  _p(counts, C.c_int32))
        return items, scores, prop, counts

    def recommend_list_propensity(self, users, lists, temperature, candidates=None, exclude=None):
        """What recommend_query_explore's policy would have given caller-given lists: ``lists`` = (offsets (M+1,)
        int64, items int32), row b's list is items[offsets[b]:offsets[b + 1]] in the order given (distinct ids, at most
        MAX_RECOMMEND).  Returns (scores, propensity), one entry per listed item: -inf / 0 where the item is no
        candidate of its row, and the rest of that list as if the item were absent.  No noise, no seed."""
        u = _i32(users)
        head = self._user_query(u, candidates, exclude)
        loff, lit = _csr(lists, len(u), "list offsets", "items")
        scores, prop = np.empty(len(lit), dtype=np.float64), np.empty(len(lit), dtype=np.float64)
        _lib.call("mmsbm_hip_recommend_list_propensity", *head, float(temperature),
                  _p(loff, C.c_int64), _p(lit, C.c_int32), _p(scores, C.c_double), _p(prop, C.c_double))
        return scores, prop

    def explore_noise(self, state, users, items):
        """(r, g) of recommend_query_explore's noise for the given (user, item) pairs of non-negative int32 ids: r the
        uniform of draw number (user << 32 | item) of the stream, g = -log(-log(1 - r)) (E = 2^-54 where r = 0),
        computed on the device by the function the perturbation calls.  Needs no session."""
        u, i = _i32(users), _i32(items)
        if u.shape != i.shape or u.ndim != 1:
            raise ValueError(f"users and items have shapes {u.shape} and {i.shape}: two 1-d arrays of one length expected")
        r, g = np.empty(len(u), dtype=np.float64), np.empty(len(u), dtype=np.float64)
        _lib.call("mmsbm_hip_explore_noise", self._h, self._pcg64_state(state), len(u), _p(u, C.c_int32),
                  _p(i, C.c_int32), _p(r, C.c_double), _p(g, C.c_double))
        return r, g

    @staticmethod
    def _categories(cat_offsets, cat_items, caps):
        """(caps int32, offsets int64, items int32) of the capped categories of the two quota queries."""
        cap = _i32(caps)
        off, it = _csr((cat_offsets, cat_items), len(cap), "category offsets", "cat_items")
        return cap, off, it

    def recommend_query_quota(self, users, n, cat_offsets, cat_items, caps, candidates=None, exclude=None):
        """recommend_query_within with per-category caps: category g holds the catalogue items
        cat_items[cat_offsets[g]:cat_offsets[g + 1]] (strictly ascending; no item in two categories; an item in none is
        uncapped) and at most caps[g] >= 0 of them enter a row's list: the row's order is walked and an item taken
        unless caps[g] items of its category were taken before it, until n are taken.  Scores and order are
        recommend_query's; without categories the answer is recommend_query_within's.  Returns what it returns."""
        u, n = _i32(users), int(n)
        head = self._user_query(u, candidates, exclude)
        cap, coff, cit = self._categories(cat_offsets, cat_items, caps)
        items, scores, counts = self._query_out(len(u), n)
        _lib.call("mmsbm_hip_recommend_query_quota", *head,
                  len(cap), _p(coff, C.c_int64), _p(cit, C.c_int32), _p(cap, C.c_int32), n,
                  _p(items, C.c_int32), _p(scores, C.c_double), _p(counts, C.c_int32))
        return items, scores, counts

    def recommend_query_theta_quota(self, theta, n, cat_offsets, cat_items, caps, seen=None, candidates=None):
        """recommend_query_theta (caller-given theta rows (S, M, K), ``seen`` lists per row, ``candidates``) with the
        per-category caps of recommend_query_quota."""
        (t, m), n = self._theta_rows(theta, self._rc_added), int(n)
        head = self._theta_query(t, m, seen, candidates)
        cap, coff, cit = self._categories(cat_offsets, cat_items, caps)
        items, scores, counts = self._query_out(m, n)
        _lib.call("mmsbm_hip_recommend_query_theta_quota", *head, len(cap), _p(coff, C.c_int64), _p(cit, C.c_int32),
                  _p(cap, C.c_int32), n, _p(items, C.c_int32), _p(scores, C.c_double), _p(counts, C.c_int32))
        return items, scores, counts

    @staticmethod
    def _shelves_out(m, n_shelves, per_shelf):
        """The empty outputs of a shelves query of m rows and their pointers (the last three null at per_shelf 0)."""
        ns, ps = max(int(n_shelves), 0), max(int(per_shelf), 0)
        out = (np.empty((m, ns), dtype=np.int32), np.empty((m, ns), dtype=np.float64), np.empty((m, ns), dtype=np.int32),
               np.empty(m, dtype=np.int32), np.empty((m, ns, ps), dtype=np.int32),
               np.empty((m, ns, ps), dtype=np.float64), np.empty((m, ns), dtype=np.int32))
        types = (C.c_int32, C.c_double, C.c_int32, C.c_int32, C.c_int32, C.c_double, C.c_int32)
        ptrs = [_p(a, t) for a, t in zip(out, types)]
        if ps == 0:
            ptrs[4:] = [None, None, None]
            out[6][:] = 0
        return out, ptrs

    def recommend_query_shelves(self, users, cat_offsets, cat_items, depth, min_items, n_shelves, per_shelf,
                                candidates=None, exclude=None):
        """Category-level recommendation: which categories to show each encoded user id, and each one's best items.
        Category g holds the catalogue items cat_items[cat_offsets[g]:cat_offsets[g + 1]] (strictly ascending; no item
        in two categories).  Over recommend_query_within's candidates (``candidates``, ``exclude`` as there) a
        category's value is the sequential mean of its min(depth, available) best scores; categories with fewer than
        min_items candidates are left out; the n_shelves best values win, equal values by ascending category index.
        Returns (categories (M,S) int32 padded with -1, values (M,S) padded with -inf, available (M,S) padded with 0,
        counts (M,), items (M,S,P) int32 padded with -1, scores (M,S,P) padded with -inf, item_counts (M,S)) for
        S = n_shelves, P = per_shelf (P = 0: the shelves only)."""
        u = _i32(users)
        head = self._user_query(u, candidates, exclude)
        coff = np.ascontiguousarray(cat_offsets, dtype=np.int64)
        coff, cit = _csr((coff, cat_items), len(coff) - 1, "category offsets", "cat_items")
        out, ptrs = self._shelves_out(len(u), n_shelves, per_shelf)
        _lib.call("mmsbm_hip_recommend_query_shelves", *head,
                  len(coff) - 1, _p(coff, C.c_int64), _p(cit, C.c_int32), int(depth), int(min_items), int(n_shelves),
                  int(per_shelf), *ptrs)
        return out

    def recommend_query_theta_shelves(self, theta, cat_offsets, cat_items, depth, min_items, n_shelves, per_shelf,
                                      seen=None, candidates=None):
        """recommend_query_shelves for caller-given theta rows (S, M, K) with ``seen`` lists per row and ``candidates``,
        as recommend_query_theta."""
        t, m = self._theta_rows(theta, self._rc_added)
        head = self._theta_query(t, m, seen, candidates)
        coff = np.ascontiguousarray(cat_offsets, dtype=np.int64)
        coff, cit = _csr((coff, cat_items), len(coff) - 1, "category offsets", "cat_items")
        out, ptrs = self._shelves_out(m, n_shelves, per_shelf)
        _lib.call("mmsbm_hip_recommend_query_theta_shelves", *head, len(coff) - 1, _p(coff, C.c_int64),
                  _p(cit, C.c_int32), int(depth), int(min_items), int(n_shelves), int(per_shelf), *ptrs)
        return out

    def recommend_rank(self, users, offsets, items, n):
        """The order of caller-given candidates, one list per request row: row b's candidates are
        items[offsets[b]:offsets[b + 1]] (ascending, distinct item ids of the session's catalogue) for encoded user
        users[b].  Returns recommend_query's triple: the n best of each list, without what recommend_query leaves
        out for the user; scores and order are recommend_query's, bit for bit."""
        u, n = _i32(users), int(n)
        off, it = _csr((offsets, items), len(u), "offsets", "items")
        out, scores, counts = self._query_out(len(u), n)
        _lib.call("mmsbm_hip_recommend_rank", self._h, len(u), _p(u, C.c_int32), _p(off, C.c_int64),
                  _p(it, C.c_int32), n, _p(out, C.c_int32), _p(scores, C.c_double), _p(counts, C.c_int32))
        return out, scores, counts

    def recommend_positions(self, users, offsets, items):
        """(positions, candidates): the position (1 = best, 0 = not a candidate) of each item in its user's full
        order within the open session -- user b's items are items[offsets[b]:offsets[b + 1]] -- and each user's
        number of candidates.  positions: (offsets[-1],) int32; candidates: (len(users),) int32."""
        u = _i32(users)
        off, it = _csr((offsets, items), len(u), "offsets", "items")
        positions = np.empty(len(it), dtype=np.int32)
        candidates = np.empty(len(u), dtype=np.int32)
        _lib.call("mmsbm_hip_recommend_positions", self._h, len(u), _p(u, C.c_int32), _p(off, C.c_int64),
                  _p(it, C.c_int32), _p(positions, C.c_int32), _p(candidates, C.c_int32))
        return positions, candidates

    def recommend_add_items(self, eta, seen=None):
        """Append new items to the open session's catalogue: eta (S, n_new, L), one (n_new, L) block per added slot in
        add order; new item j gets id n_items + j.  seen: None or (offsets (n_new+1,) int64, users int32): the training
        users that rated new item j are users[offsets[j]:offsets[j + 1]], and that pair is left out of their lists.
        Once per session, after every recommend_add."""
        e = _slot_blocks(eta, "eta", f"expected (slots, items, {self.l})", self.l, self._rc_added)
        n_new = e.shape[1]
        _lib.call("mmsbm_hip_recommend_add_items", self._h, n_new, _p(e, C.c_double),
                  *_row_csr(seen, n_new, "seen offsets", "users"))

    MAX_TOP_PAIRS = 1024

    def recommend_top_pairs(self, m, users=None):
        """(users (m,) int32, items (m,) int32, scores (m,), count): the m best (user, item) pairs of the open session
        over the encoded user ids ``users`` (distinct; None: every training user) -- score descending, equal scores
        by ascending user id, then item id; entries behind ``count`` are -1 / -1 / -inf."""
        m = int(m)
        ou, oi = np.empty(max(m, 0), dtype=np.int32), np.empty(max(m, 0), dtype=np.int32)
        sc = np.empty(max(m, 0), dtype=np.float64)
        count = C.c_int32(0)
        _lib.call("mmsbm_hip_recommend_top_pairs", self._h, *_user_set(users, 0), m, _p(ou, C.c_int32), _p(oi, C.c_int32),
                  _p(sc, C.c_double), C.byref(count))
        return ou, oi, sc, int(count.value)

    MAX_TOP_PAIRS_BULK = 1 << 26

    def recommend_top_pairs_bulk(self, m, users=None):
        """(users (m,) int32, items (m,) int32, scores (m,), count, info): recommend_top_pairs' answer for m up to
        MAX_TOP_PAIRS_BULK, found by a radix select of the bar over the score tiles.  info: {"bar": the score of the
        last returned pair, "above" / "ties": candidates that score strictly above / exactly the bar, "candidates"}."""
        m = int(m)
        ou, oi = np.empty(max(m, 0), dtype=np.int32), np.empty(max(m, 0), dtype=np.int32)
        sc = np.empty(max(m, 0), dtype=np.float64)
        count, bar, counts = C.c_int64(0), C.c_double(0.0), np.zeros(3, dtype=np.int64)
        _lib.call("mmsbm_hip_recommend_top_pairs_bulk", self._h, *_user_set(users, 0), m, _p(ou, C.c_int32),
                  _p(oi, C.c_int32), _p(sc, C.c_double), C.byref(count), C.byref(bar), _p(counts, C.c_int64))
        return ou, oi, sc, int(count.value), self._bar_info(bar, counts)

    def recommend_pair_bar(self, m, users=None):
        """recommend_top_pairs_bulk's info alone: the select and one counting pass, no entries."""
        bar, counts = C.c_double(0.0), np.zeros(3, dtype=np.int64)
        _lib.call("mmsbm_hip_recommend_pair_bar", self._h, *_user_set(users, 0), int(m), C.byref(bar), _p(counts, C.c_int64))
        return self._bar_info(bar, counts)

    @staticmethod
    def _bar_info(bar, counts):
        return {"bar": float(bar.value), "above": int(counts[0]), "ties": int(counts[1]), "candidates": int(counts[2])}

    def recommend_query_items(self, items, n):
        """(users (M,n) int32 padded with -1, scores (M,n) padded with -inf, counts (M,)) for item ids of the open
        session's catalogue: the n best candidate users of each -- score descending, equal scores by ascending user
        id; the pair (u, i) is left out exactly when recommend_query leaves i out for u."""
        return self._top_n("mmsbm_hip_recommend_query_items", items, n)

    def recommend_allocate(self, users, n, caps, max_rounds=10000):
        """Capacity-aware allocation inside the open session: every user of ``users`` (distinct encoded ids; None: all
        training users) asks for n items, item i of the session's catalogue can be given out caps[i] times (0: not at
        all, negative: unlimited).  The answer is the walk over all candidate pairs in top_pairs' order that takes a
        pair iff its user holds fewer than n items and its item is not used up.  Returns (items, scores, counts) as
        recommend_query -- a row may hold fewer than n -- and {"rounds", "converged"}: the rounds of deferred
        acceptance it took, and whether they reached the fixed point within ``max_rounds`` (if not, the answer is
        feasible but not the walk's)."""
        (m, u), n = _user_set(users, self.n_users), int(n)
        cap = _i32(caps)
        items, scores, counts = self._query_out(m, n)
        rounds, converged = C.c_int32(0), C.c_int32(0)
        _lib.call("mmsbm_hip_recommend_allocate", self._h, m, u, n, _p(cap, C.c_int32),
                  int(max_rounds), _p(items, C.c_int32), _p(scores, C.c_double), _p(counts, C.c_int32),
                  C.byref(rounds), C.byref(converged))
        return items, scores, counts, {"rounds": int(rounds.value), "converged": bool(converged.value)}

    def recommend_assign(self, users, caps, reserve, epsilon, max_rounds=10000):
        """Welfare-maximising assignment inside the open session: every user of ``users`` (distinct encoded ids; None:
        all training users) gets at most one item, item i of the session's catalogue at most caps[i] users (0: none,
        negative: unlimited), and the sum of the assigned scores plus ``reserve`` per unassigned user is the largest
        possible within (assigned users) x ``epsilon`` -- a forward auction on the device.  Returns a dict: by request
        row ``items`` (-1: unassigned), ``scores`` (-inf), ``paid``, ``pi``; by catalogue item ``price`` (its cheapest
        slot), ``price_sum``, ``load``; and ``rounds``, ``bids``, ``converged``.  sum(pi) + sum(price_sum) bounds the
        optimum from above."""
        m, u = _user_set(users, self.n_users)
        cap = _i32(caps)
        if cap.ndim != 1 or len(cap) < self.n_items:
            raise ValueError(f"caps has shape {cap.shape}, expected one entry per item of the session's catalogue")
        items = np.full(m, -1, dtype=np.int32)
        scores, paid, pi = (np.empty(m, dtype=np.float64) for _ in range(3))
        price, price_sum = np.empty(len(cap), dtype=np.float64), np.empty(len(cap), dtype=np.float64)
        load = np.zeros(len(cap), dtype=np.int32)
        rounds, converged = C.c_int32(0), C.c_int32(0)
        _lib.call("mmsbm_hip_recommend_assign", self._h, m, u, _p(cap, C.c_int32), float(reserve),
                  float(epsilon), int(max_rounds), _p(items, C.c_int32), _p(scores, C.c_double), _p(paid, C.c_double),
                  _p(pi, C.c_double), _p(price, C.c_double), _p(price_sum, C.c_double), _p(load, C.c_int32),
                  C.byref(rounds), C.byref(converged))
        return {"items": items, "scores": scores, "paid": paid, "pi": pi, "price": price, "price_sum": price_sum,
                "load": load, "rounds": int(rounds.value), "converged": bool(converged.value),
                "bids": int(self.get_option("assign_bids"))}

    def recommend_audience(self, items, min_score, count_only=False, total=None):
        """(offsets (M+1,) int64, users int32, scores): for each item id every candidate user whose score is >=
        min_score, in ascending user id -- item b's are [offsets[b]:offsets[b + 1]].  A sizes call followed by a
        filled call; with count_only only the first, and users / scores are None.  ``total``: offsets[-1] of an
        earlier sizes call for the same request, which is then not made again."""
        i = _i32(items)
        offsets = np.zeros(len(i) + 1, dtype=np.int64)
        args = (self._h, len(i), _p(i, C.c_int32), float(min_score))
        if total is None or count_only:
            _lib.call("mmsbm_hip_recommend_audience", *args, 0, _p(offsets, C.c_int64), None, None)
            if count_only:
                return offsets, None, None
            total = int(offsets[-1])
        users, scores = np.empty(total, dtype=np.int32), np.empty(total, dtype=np.float64)
        _lib.call("mmsbm_hip_recommend_audience", *args, total, _p(offsets, C.c_int64), _p(users, C.c_int32),
                  _p(scores, C.c_double))
        return offsets, users, scores

    def recommend_end(self):
        _lib.call("mmsbm_hip_recommend_end", self._h)

    # -- nearest items / users on the device (include/mmsbm_hip.h: mmsbm_hip_similar_*) -----------------
    def similar_begin(self, side):
        """Open a similarity session over one side: 0 (or "items") the items, 1 (or "users") the users."""
        side = {"items": 0, "users": 1}.get(side, side)
        _lib.call("mmsbm_hip_similar_begin", self._h, int(side))

    def similar_add(self):
        """Add the selected slot's rating profiles and group masses to the session (the slot is left unchanged)."""
        _lib.call("mmsbm_hip_similar_add", self._h)

    def similar_query(self, ids, n):
        """(ids (M,n) int32 padded with -1, distance (M,n) padded with +inf, counts (M,)) for encoded ids of the
        session's side: the n nearest other rows of each, distance ascending, equal distances by ascending id."""
        return self._top_n("mmsbm_hip_similar_query", ids, n)

    def similar_end(self):
        _lib.call("mmsbm_hip_similar_end", self._h)

    def similar_pairs(self, a, b):
        """distance (M,): D(a[e], b[e]) of the open similarity session for encoded ids of its side -- similar_query's
        number for the pair, bit for bit; symmetric, +0.0 between a row and itself."""
        a, b = _i32(a), _i32(b)
        if a.shape != b.shape or a.ndim != 1:
            raise ValueError(f"a and b must be two id columns of one length, got shapes {a.shape} and {b.shape}")
        out = np.empty(len(a), dtype=np.float64)
        _lib.call("mmsbm_hip_similar_pairs", self._h, len(a), _p(a, C.c_int32), _p(b, C.c_int32), _p(out, C.c_double))
        return out

    # -- diversified top-N on the device (include/mmsbm_hip.h: mmsbm_hip_recommend_diverse) -----------------
    def recommend_diverse(self, users, n, pool, trade_off, candidates=None, exclude=None):
        """(items (M,n) int32 padded with -1, scores (M,n) padded with -inf, distances (M,n) padded with +inf, counts
        (M,)): the greedy re-ranking of each user's ``pool`` best candidates -- the row recommend_query_within(users,
        pool, candidates, exclude) returns -- by score + trade_off x (distance to the nearest item picked so far), with
        the open recommend session's scores and the distance of the open similarity session over the items (both must
        hold the same slots, added in the same order).  distances: to the nearest earlier pick, +inf for the first."""
        u, n, pool = _i32(users), int(n), int(pool)
        items, scores, counts = self._query_out(len(u), n)
        distances = np.empty((len(u), max(n, 0)), dtype=np.float64)
        _lib.call("mmsbm_hip_recommend_diverse", *self._user_query(u, candidates, exclude), n, pool,
                  float(trade_off), _p(items, C.c_int32), _p(scores, C.c_double), _p(distances, C.c_double),
                  _p(counts, C.c_int32))
        return items, scores, distances, counts

    # -- group queries of the recommend session (include/mmsbm_hip.h: mmsbm_hip_recommend_query_groups) -----
    GROUP_MODES = {"min": 0, "max": 1, "count": 2, "mean": 3}   # MMSBM_HIP_GROUP_*

    def recommend_query_groups(self, offsets, members, n, mode, bar=0.0, candidates=None):
        """(items (G,n) int32 padded with -1, scores (G,n) padded with -inf, counts (G,)) for G groups of encoded user
        ids: group g's members are members[offsets[g]:offsets[g + 1]] (distinct within a group).  ``mode`` (a key of
        GROUP_MODES or its number): "min" the lowest score a member gives the item, "max" the highest, "count" the
        number of members whose score is >= ``bar``, "mean" the score of the group's mean row.  Candidates:
        ``candidates`` (ascending, distinct item ids of the session's catalogue; None: all of it) without every item
        that recommend_query leaves out for ANY member.  Order: value descending, equal values by ascending item id.
        The members' scores are recommend_query's, bit for bit."""
        m, n = _i32(members), int(n)
        off = np.ascontiguousarray(offsets, dtype=np.int64)
        if off.ndim != 1 or len(off) < 1:
            raise ValueError(f"offsets have shape {off.shape}, expected (groups + 1,)")
        if off[-1] != len(m):
            raise ValueError(f"offsets end at {int(off[-1])}, members holds {len(m)}")
        groups = len(off) - 1
        items, scores, counts = self._query_out(groups, n)
        _lib.call("mmsbm_hip_recommend_query_groups", self._h, groups, _p(off, C.c_int64), _p(m, C.c_int32),
                  int(self.GROUP_MODES.get(mode, mode)), float(bar), *_subset(candidates), n,
                  _p(items, C.c_int32), _p(scores, C.c_double), _p(counts, C.c_int32))
        return items, scores, counts

    # -- greedy assortment selection in the recommend session (include/mmsbm_hip.h: mmsbm_hip_recommend_assortment) -----
    ASSORT_MODES = {"best_score": 0, "reach": 1}                # MMSBM_HIP_ASSORT_*
    ASSORT_STOPS = ("c", "no_gain", "no_candidates")            # MMSBM_HIP_ASSORT_STOP_*
    MAX_ASSORT = 1024                                           # MMSBM_HIP_ASSORT_MAX_C

    def recommend_assortment(self, users, c, mode, level, given=None, candidates=None):
        """(items (count,) int32, gains (count,), count, stop reason, served items (M,) int32, served scores (M,), start):
        at most ``c`` greedy rounds over the encoded ``users`` (any order; a user named twice counts once, M of them are
        distinct) -- each takes the candidate of largest gain, equal gains by the smaller id.  ``mode`` (a key of
        ASSORT_MODES or its number): "best_score" the gain of an item is the sum over the users of how far its score
        lies above the best score the user has so far (``level``: the floor that stands for "nothing"), "reach" the number
        of users not reached yet whose score is >= ``level`` (the bar).  ``given`` (encoded items, in order): applied to
        the state first and never chosen; ``start``: the gain they had together.  ``candidates`` as in
        recommend_query_within.  gains: per round, the sum divided by S.  The served arrays stand in the order of the
        users' first appearance: the item that serves each user (-1: none) and its score (-inf), read from the state on
        the device.  Stop reason: one of ASSORT_STOPS."""
        u, c = _i32(users), int(c)
        uniq, first = np.unique(u, return_index=True)
        uniq = np.ascontiguousarray(uniq, dtype=np.int32)
        place = np.searchsorted(uniq, u[np.sort(first)])       # the sorted row of every distinct user, first appearance first
        g = _i32([] if given is None else given)
        items = np.full(max(c, 0), -1, dtype=np.int32)
        gains = np.zeros(max(c, 0), dtype=np.float64)
        given_gains = np.zeros(len(g), dtype=np.float64)
        count, stop = np.zeros(1, dtype=np.int32), np.zeros(1, dtype=np.int32)
        s_items = np.full(len(uniq), -1, dtype=np.int32)
        s_scores = np.full(len(uniq), -np.inf, dtype=np.float64)
        _lib.call("mmsbm_hip_recommend_assortment", self._h, len(uniq), _p(uniq, C.c_int32),
                  int(self.ASSORT_MODES.get(mode, mode)), float(level), len(g), _p(g, C.c_int32),
                  *_subset(candidates), c, _p(items, C.c_int32),
                  _p(gains, C.c_double), _p(count, C.c_int32), _p(stop, C.c_int32), _p(given_gains, C.c_double),
                  _p(s_items, C.c_int32), _p(s_scores, C.c_double))
        n = int(count[0])
        start = float(np.cumsum(given_gains)[-1]) if len(g) else 0.0      # (added in the order given)
        return items[:n], gains[:n], n, self.ASSORT_STOPS[int(stop[0])], s_items[place], s_scores[place], start

    # -- ensemble-aware queries of the recommend session (include/mmsbm_hip.h: mmsbm_hip_recommend_query_ensemble) -----
    ENSEMBLE_MODES = {"min": 0, "max": 1, "lcb": 2}   # MMSBM_HIP_ENSEMBLE_*

    def recommend_query_ensemble(self, users, n, mode, risk=0.0, candidates=None, exclude=None):
        """recommend_query_within -- the same candidates, exclusions and output -- with a pair valued by how the added
        slots agree on it.  ``mode`` (a key of ENSEMBLE_MODES or its number): "min" the lowest score a slot alone gives
        the pair, "max" the highest, "lcb" mean - ``risk`` x std over the slots (population std; ``risk`` 0: the mean,
        negative: exploration).  With one slot added every mode answers as recommend_query, bit for bit."""
        u, n = _i32(users), int(n)
        items, scores, counts = self._query_out(len(u), n)
        head = self._user_query(u, candidates, exclude)   # (the mode and the risk stand behind the users)
        _lib.call("mmsbm_hip_recommend_query_ensemble", *head[:3], int(self.ENSEMBLE_MODES.get(mode, mode)), float(risk),
                  *head[3:], n,
                  _p(items, C.c_int32), _p(scores, C.c_double), _p(counts, C.c_int32))
        return items, scores, counts

    def recommend_pair_spread(self, users, items, per_slot=False):
        """stats (M, 4): mean, std, worst, best over the added slots of the score each slot alone gives the pair
        (users[e], items[e]) -- encoded ids of training users and of the session's catalogue -- the bits
        recommend_query_ensemble ranks by.  With ``per_slot``: (stats, (S, M) every slot's own score)."""
        u, i = _i32(users), _i32(items)
        if u.shape != i.shape or u.ndim != 1:
            raise ValueError(f"users and items must be two id columns of one length, got shapes {u.shape} and {i.shape}")
        stats = np.empty((len(u), 4), dtype=np.float64)
        each = np.empty((self._rc_added, len(u)), dtype=np.float64) if per_slot else None
        _lib.call("mmsbm_hip_recommend_pair_spread", self._h, len(u), _p(u, C.c_int32), _p(i, C.c_int32),
                  _p(stats, C.c_double), _p_or_null(each, C.c_double))
        return (stats, each) if per_slot else stats

    # -- the items whose rating tells most about a user (include/mmsbm_hip.h: mmsbm_hip_inform_*) ---------
    def inform_begin(self):
        """Open an inform session: the information gain of a rating, averaged over the slots added to it."""
        _lib.call("mmsbm_hip_inform_begin", self._h)
        self._inf_added = 0

    def inform_add(self):
        """Add the selected slot's theta rows, item profiles and their entropies to the session (the slot is left
        unchanged)."""
        _lib.call("mmsbm_hip_inform_add", self._h)
        self._inf_added += 1

    def inform_query(self, users, n, candidates=None, exclude=None, exclude_seen=True):
        """(items (M,n) int32 padded with -1, gain (M,n) padded with -inf, counts (M,)) for encoded user ids: the n items
        whose rating would tell most about the group the user acts from -- gain descending, equal gains by ascending
        item id -- among ``candidates`` (ascending, distinct item ids; None: every item), without the user's training
        items when ``exclude_seen`` and without ``exclude``: None or (offsets (M+1,) int64, items int32), request row b
        also leaves out items[offsets[b]:offsets[b + 1]]."""
        u, n = _i32(users), int(n)
        items, gains, counts = self._query_out(len(u), n)
        _lib.call("mmsbm_hip_inform_query", *self._user_query(u, candidates, exclude), int(bool(exclude_seen)), n,
                  _p(items, C.c_int32), _p(gains, C.c_double), _p(counts, C.c_int32))
        return items, gains, counts

    def inform_query_theta(self, theta, n, seen=None, candidates=None):
        """inform_query for caller-given users: theta (S, M, K), one (M, K) block per added slot in add order, entries
        finite and >= 0.  seen: None (nothing excluded) or (offsets (M+1,) int64, items int32): user b leaves out
        items[offsets[b]:offsets[b + 1]].  candidates as in inform_query."""
        (t, m), n = self._theta_rows(theta, getattr(self, "_inf_added", 0)), int(n)
        head = self._theta_query(t, m, seen, candidates)
        items, gains, counts = self._query_out(m, n)
        _lib.call("mmsbm_hip_inform_query_theta", *head, n,
                  _p(items, C.c_int32), _p(gains, C.c_double), _p(counts, C.c_int32))
        return items, gains, counts

    def inform_mean_theta(self):
        """(S, K): the mean theta row of the training users under each added slot, in add order."""
        out = np.empty((getattr(self, "_inf_added", 0), self.k), dtype=np.float64)
        _lib.call("mmsbm_hip_inform_mean_theta", self._h, _p(out, C.c_double) if out.size else None)
        return out

    def inform_end(self):
        _lib.call("mmsbm_hip_inform_end", self._h)
        self._inf_added = 0

    # -- the overlap of the restarts' groups on the device (include/mmsbm_hip.h: mmsbm_hip_overlap_*) ----
    def overlap_begin(self, side):
        """Open an overlap session over one side: 0 (or "items") eta's L groups, 1 (or "users") theta's K groups."""
        side = {"items": 0, "users": 1}.get(side, side)
        _lib.call("mmsbm_hip_overlap_begin", self._h, int(side))
        self._ov = [self.l if int(side) == 0 else self.k, 0]   # (groups, slots added)

    def overlap_add(self):
        """Add the selected slot's membership table of the session's side (the slot is left unchanged)."""
        _lib.call("mmsbm_hip_overlap_add", self._h)
        self._ov[1] += 1

    def overlap_query(self):
        """(F, F) with F = slots added x groups: entry (s G + a, t G + b) is the sum over the rows of
        x_s[row, a] x_t[row, b]."""
        groups, slots = getattr(self, "_ov", None) or (0, 0)
        f = groups * slots
        out = np.empty((f, f), dtype=np.float64)
        _lib.call("mmsbm_hip_overlap_query", self._h, _p(out, C.c_double) if f else None)
        return out

    def overlap_end(self):
        _lib.call("mmsbm_hip_overlap_end", self._h)
        self._ov = None

    # -- which of a user's training rows carry a recommendation (include/mmsbm_hip.h: mmsbm_hip_explain_*) ----
    def explain_begin(self, rating_weights):
        """Open an explain session: the attribution of score = sum_r w_r P(r | u, i), averaged over the slots added to
        it, to the user's training rows."""
        w = _f64(rating_weights)
        if w.shape != (self.n_ratings,):
            raise ValueError(f"rating_weights has shape {w.shape}, expected ({self.n_ratings},)")
        _lib.call("mmsbm_hip_explain_begin", self._h, _p(w, C.c_double))

    def explain_add(self):
        """Add the selected slot's current parameters to the session (the slot is left unchanged)."""
        _lib.call("mmsbm_hip_explain_add", self._h)

    def explain_query(self, users, offsets, items, n):
        """For encoded user ids, user b with the candidate items items[offsets[b]:offsets[b + 1]]; pair q counted in that
        flattened order: (hist_items (Q,n) int32 padded with -1, hist_ratings (Q,n) int32 padded with -1, contribution
        (Q,n) padded with -inf, counts (Q,), explained (Q,), score (Q,), degree (Q,)) -- the n training rows of the
        pair's user that carry most of the pair's score, contribution descending, equal ones by ascending item id, then
        rating id; explained: the sum over ALL the user's rows."""
        u, n = _i32(users), int(n)
        off, it = _csr((offsets, items), len(u), "offsets", "items")
        q = len(it)
        hi, hr = np.empty((q, max(n, 0)), dtype=np.int32), np.empty((q, max(n, 0)), dtype=np.int32)
        co = np.empty((q, max(n, 0)), dtype=np.float64)
        counts, degree = np.empty(q, dtype=np.int32), np.empty(q, dtype=np.int32)
        explained, score = np.empty(q, dtype=np.float64), np.empty(q, dtype=np.float64)
        _lib.call("mmsbm_hip_explain_query", self._h, len(u), _p(u, C.c_int32), _p(off, C.c_int64), _p(it, C.c_int32), n,
                  _p(hi, C.c_int32), _p(hr, C.c_int32), _p(co, C.c_double), _p(counts, C.c_int32),
                  _p(explained, C.c_double), _p(score, C.c_double), _p(degree, C.c_int32))
        return hi, hr, co, counts, explained, score, degree

    def explain_end(self):
        _lib.call("mmsbm_hip_explain_end", self._h)

    # -- leave-one-out reliability of the training rows (include/mmsbm_hip.h: mmsbm_hip_loo_*) ----
    MAX_LOO_M = 1024

    def loo_begin(self):
        """Open a leave-one-out session over the training rows: the probability of each row's rating under parameters
        that never saw the row, averaged over the slots added to it."""
        _lib.call("mmsbm_hip_loo_begin", self._h)

    def loo_add(self):
        """Add the selected slot's current parameters to the session (the slot is left unchanged)."""
        _lib.call("mmsbm_hip_loo_add", self._h)

    def loo_rows(self, rows=None):
        """(fitted, reliability) at the positions ``rows`` of the training table (None: every row, in training order):
        the in-sample and the leave-one-out probability of the row's rating, means over the slots added."""
        if rows is None:
            n, pos = self.n_obs, None
        else:
            pos = np.ascontiguousarray(rows, dtype=np.int64).reshape(-1)
            n = len(pos)
        fitted, rel = np.empty(n, dtype=np.float64), np.empty(n, dtype=np.float64)
        if pos is not None and n == 0:   # (an empty array has no address to tell from "every row")
            pos = np.zeros(1, dtype=np.int64)
        _lib.call("mmsbm_hip_loo_rows", self._h, n, _p_or_null(pos, C.c_int64), _p(fitted, C.c_double),
                  _p(rel, C.c_double))
        return fitted, rel

    def loo_sides(self):
        """(user surprise (U,), user fitted_surprise (U,), item surprise (I,), item fitted_surprise (I,)): the mean of
        -log(max(reliability, eps)) -- and of the same built from fitted -- over each user's and each item's training
        rows; NaN where there are none."""
        out = [np.empty(n, dtype=np.float64) for n in (self.n_users, self.n_users, self.n_items, self.n_items)]
        _lib.call("mmsbm_hip_loo_sides", self._h, *[_p(a, C.c_double) for a in out])
        return tuple(out)

    def loo_lowest(self, m, user_flags=None, item_flags=None):
        """(rows (m,) int64 padded with -1, reliability (m,) padded with +inf, count): the ``m`` training rows of
        smallest reliability -- ascending, exactly equal ones by ascending position -- among the rows whose user is
        flagged in ``user_flags`` ((U,) bool; None: every user) and whose item is flagged in ``item_flags``."""
        m = int(m)
        flags = []
        for given, size, name in ((user_flags, self.n_users, "user_flags"), (item_flags, self.n_items, "item_flags")):
            if given is not None:
                given = np.ascontiguousarray(np.asarray(given) != 0, dtype=np.uint8)
                if given.shape != (size,):
                    raise ValueError(f"{name} has shape {given.shape}, expected ({size},)")
            flags.append(given)
        rows, rel = np.empty(max(m, 0), dtype=np.int64), np.empty(max(m, 0), dtype=np.float64)
        count = C.c_int32(0)
        _lib.call("mmsbm_hip_loo_lowest", self._h, m, _p_or_null(flags[0], C.c_uint8), _p_or_null(flags[1], C.c_uint8),
                  _p(rows, C.c_int64), _p(rel, C.c_double), C.byref(count))
        return rows, rel, int(count.value)

    def loo_end(self):
        _lib.call("mmsbm_hip_loo_end", self._h)

    # -- held-out log-likelihood and snapshots on the device (include/mmsbm_hip.h: mmsbm_hip_heldout_*) ----
    def heldout_begin(self, rows):
        """Open a held-out session over (M,3) triples [user, item, observed rating index] (encoded ids)."""
        u, i, r = split_triples(rows)
        _lib.call("mmsbm_hip_heldout_begin", self._h, len(u), _p(u, C.c_int32), _p(i, C.c_int32), _p(r, C.c_int32))
        self._ho_rows = len(u)   # (only now: a refused begin leaves an earlier session, and its row count, as they are)

    def heldout_eval(self):
        """(slots,) sum over the rows of log P(observed rating | user, item) under EVERY slot's current parameters,
        in one set of launches; changes nothing."""
        out = np.zeros(self.slots, dtype=np.float64)
        _lib.call("mmsbm_hip_heldout_eval", self._h, _p(out, C.c_double))
        return out

    def heldout_add(self):
        """The selected slot's held-out log-likelihood; its row probabilities join the session's running sum."""
        out = C.c_double(0.0)
        _lib.call("mmsbm_hip_heldout_add", self._h, C.byref(out))
        return np.float64(out.value)

    def heldout_mean(self, want_rows=True):
        """(mean row probability over the slots added (M,) in request order or None, its log-likelihood)."""
        out = C.c_double(0.0)
        mean = np.empty(self._ho_rows, dtype=np.float64) if want_rows else None
        _lib.call("mmsbm_hip_heldout_mean", self._h, _p(mean, C.c_double) if want_rows else None, C.byref(out))
        return mean, np.float64(out.value)

    def heldout_end(self):
        _lib.call("mmsbm_hip_heldout_end", self._h)

    def snapshot_save(self):
        """Keep the selected slot's current parameters on the device (replaces that slot's earlier snapshot)."""
        _lib.call("mmsbm_hip_snapshot_save", self._h)

    def snapshot_get(self):
        """(theta, eta, pr) of the selected slot's snapshot."""
        theta, eta, pr = (np.empty(s, dtype=np.float64) for s in self._shapes())
        _lib.call("mmsbm_hip_snapshot_get", self._h, _p(theta, C.c_double), _p(eta, C.c_double), _p(pr, C.c_double))
        return theta, eta, pr

    # -- fold-in of new users (include/mmsbm_hip.h: mmsbm_hip_fold_in) ---------------------------------
    MAX_FOLD_IN_K = 1024

    def fold_in(self, rows, n_new, iterations, tol=None, theta0=None):
        """theta (n_new, K) of new users 0 .. n_new-1 under the selected slot's eta and p, and the iterations each ran
        (n_new,).  rows: (N, 3) [new user, item, rating] (encoded item and rating ids).  tol None: all iterations;
        theta0 None: uniform 1/K.  The slot is left unchanged."""
        return self._fold("mmsbm_hip_fold_in", self.k, "theta0", rows, n_new, iterations, tol, theta0)

    def fold_in_items(self, rows, n_new, iterations, tol=None, eta0=None):
        """eta (n_new, L) of new items 0 .. n_new-1 under the selected slot's theta and p, and the iterations each ran
        (n_new,).  rows: (N, 3) [user, new item, rating] (encoded user and rating ids, training data's column order).
        tol None: all iterations; eta0 None: uniform 1/L.  The slot is left unchanged."""
        return self._fold("mmsbm_hip_fold_in_items", self.l, "eta0", rows, n_new, iterations, tol, eta0)

    def _fold(self, symbol, groups, start_name, rows, n_new, iterations, tol, start):
        """fold_in / fold_in_items through ABI entry ``symbol``: rows of ``groups`` columns, ``start`` (named
        ``start_name``) or None."""
        u, i, r = split_triples(rows)
        n_new = int(n_new)
        if start is not None:
            start = _f64(start)
            if start.shape != (n_new, groups):
                raise ValueError(f"{start_name} has shape {start.shape}, expected ({n_new}, {groups})")
        out = np.empty((n_new, groups), dtype=np.float64)
        iters = np.empty(n_new, dtype=np.int32)
        _lib.call(symbol, self._h, len(u), _p(u, C.c_int32), _p(i, C.c_int32), _p(r, C.c_int32),
                  n_new, int(iterations), -1.0 if tol is None else float(tol),
                  _p_or_null(start, C.c_double), _p(out, C.c_double), _p(iters, C.c_int32))
        return out, iters

    # -- measurement -------------------------------------------------------------------------
    def time_iterations(self, n_iters):
        """Device milliseconds for n_iters EM iterations (HIP events on the context stream)."""
        ms = C.c_float(0.0)
        _lib.call("mmsbm_hip_time_iterations", self._h, int(n_iters), C.byref(ms))
        return float(ms.value)

    def profile_iterations(self, n_iters):
        """{kernel name: (mean microseconds per launch, launches per iteration, bytes read,
        bytes written)} from a HIP event pair around every launch."""
        lib = _lib.load()
        nk = lib.mmsbm_hip_kernel_count()
        us = (C.c_float * nk)()
        cnt = (C.c_int * nk)()
        _lib.call("mmsbm_hip_profile_iterations", self._h, int(n_iters), us, cnt)
        out = {}
        for j in range(nk):
            rd, wr = C.c_int64(0), C.c_int64(0)
            _lib.call("mmsbm_hip_kernel_bytes", self._h, j, C.byref(rd), C.byref(wr))
            out[lib.mmsbm_hip_kernel_name(j).decode()] = (float(us[j]), int(cnt[j]),
                                                         int(rd.value), int(wr.value))
        return out

    def time_stage(self, stage, reps=50):
        """Mean microseconds of `reps` back-to-back launches of one stage (clobbers state)."""
        us = C.c_float(0.0)
        _lib.call("mmsbm_hip_time_stage", self._h, int(stage), int(reps), C.byref(us))
        return float(us.value)

    def set_option(self, name, value):
        """Set a named option of the library (mmsbm_hip_set_option in include/mmsbm_hip.h lists them); a name that can
        only be read is refused like an unknown one."""
        _lib.call("mmsbm_hip_set_option", self._h, name.encode(), float(value))

    def get_option(self, name):
        v = C.c_double(0.0)
        _lib.call("mmsbm_hip_get_option", self._h, name.encode(), C.byref(v))
        return float(v.value)

    def set_graph_mode(self, mode):
        """0 eager launches (default), 1 replay a captured hipGraph of two iterations."""
        _lib.call("mmsbm_hip_set_graph_mode", self._h, int(mode))

    def index_arrays(self):
        """The index this context's kernels read (mmsbm_hip_index_array), read back from the device where it lives
        there: the names of ``build_layout`` plus ``item_grid``, ``lik_units`` and ``mv_chunk_off``.  Internal terms:
        in a swapped context the "users" are the caller's items."""
        out = {}
        for which, nm in enumerate(LAYOUT_NAMES + INDEX_ONLY_NAMES):
            arr = _fetch_i32("mmsbm_hip_index_array", self._h, which)
            out[nm] = arr.reshape(-1, 4) if nm in RECORD_NAMES else arr
        return out


def build_layout(data, n_users, n_items, n_ratings, target_chunks=1024, fused_caps=None):
    """Host-only: the sorted CSR layout the library uploads (dict of int32 arrays).  ``fused_caps = (pair cap, user
    cap)`` adds the whole-segment lists of the two-launch iteration (mmsbm_hip_layout_fused): ``fused_pairs`` /
    ``fused_users`` = {"units", "items", "splits", "chunks", "max_parts", "built"}."""
    u, i, r = split_triples(data)
    h = C.c_void_p()
    _lib.call("mmsbm_hip_layout_build", len(u), int(n_users), int(n_items), int(n_ratings),
              _p(u, C.c_int32), _p(i, C.c_int32), _p(r, C.c_int32), int(target_chunks), C.byref(h))
    out = {}
    try:
        for which, nm in enumerate(LAYOUT_NAMES):
            arr = _fetch_i32("mmsbm_hip_layout_array", h, which)
            out[nm] = arr.reshape(-1, 4) if which >= 10 else arr
        if fused_caps is not None:
            for side, (key, cap) in enumerate(zip(("fused_pairs", "fused_users"), fused_caps)):
                rec = {}
                for which, nm in enumerate(("units", "items", "splits", "chunks", "info")):
                    arr = _fetch_i32("mmsbm_hip_layout_fused", h, side, int(cap), which)
                    rec[nm] = arr.reshape(-1, 4) if which < 4 else arr
                rec["max_parts"], rec["built"] = int(rec["info"][0]), bool(rec["info"][1])
                out[key] = rec
    finally:
        _lib.call("mmsbm_hip_layout_free", h)
    return out
