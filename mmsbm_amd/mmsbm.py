"""Host class with the surface of the reference's ``MMSBM`` (src/mmsbm.py:15-553) for
``backend='hip'``: same constructor keywords, ``fit`` / ``predict`` / ``score`` / ``cv_fit``,
``results`` as a list of ``{"likelihood", "pr", "theta", "eta"}`` dicts in restart order.

What differs from the reference is where things run: the whole EM loop of a restart stays on
the GPU (src/mmsbm.py:243-250 becomes one C-ABI call), the restarts that share a GPU advance
together as the slots of one ``HipEM`` context (one set of kernel launches per iteration
for all of them: the batching the reference lists as a TODO, README.md:188), and restarts
are spread over GPUs -- threads over ``devices`` inside one process, or ranks of a
``torch.distributed`` job (mmsbm_amd/restarts.py) -- instead of a ``multiprocessing.Pool``
(src/mmsbm.py:182-185).  Restart ``i`` is seeded exactly like the reference
(``SeedSequence(seed).spawn(sampling)[i]``, draw order theta, eta, p) and slots never
interact, so its result does not depend on ``sampling``, on the batch it ran in or on
which GPU ran it.
"""
from __future__ import annotations

import contextlib
import logging
from concurrent.futures import ThreadPoolExecutor
from datetime import datetime

import numpy as np

from .backend import load_backend
from ._lib import HipLibraryError
from .core import HipEM, data_key, normalize_with_self  # noqa: F401  (re-exported)
from .encode import Encoder


class MMSBM:
    data_handler = None
    results = None
    test = None
    theta = None
    eta = None
    pr = None
    likelihood = None
    prediction_matrix = None
    rng = None

    def __init__(self, user_groups, item_groups, iterations=400, sampling=1, seed=None,
                 debug=False, backend="auto", devices=None, restarts_per_launch=None,
                 contexts_per_device=1, tol=None, check_every=50):
        self.start_time = datetime.now()
        self.user_groups = user_groups
        self.item_groups = item_groups
        self.iterations = iterations
        self.sampling = sampling
        self.debug = debug
        self.backend = backend
        self.devices = devices
        # Restarts that share a GPU run as slots of one context, up to this many per batch
        # (C3: 1.2x the restarts/s of one at a time, C2: 3x, C1-sized problems: ~Sx).
        # restarts advanced together as slots of one context; None: HipEM.suggested_slots() decides from the table sizes
        self.restarts_per_launch = None if restarts_per_launch is None else max(1, int(restarts_per_launch))
        # More than one context (= stream) per GPU is possible too; slots do the same job
        # better, so the default is one.
        self.contexts_per_device = max(1, int(contexts_per_device))
        # Convergence monitor (not in the reference, off by default): every `check_every`
        # iterations the likelihood of each restart of the batch is evaluated -- the reference's
        # debug hook, src/mmsbm.py:252-254 -- and with `tol` set the batch stops early once every
        # restart's relative change is below it.  `iterations_run[i]` records what restart i got.
        self.tol = tol
        self.check_every = max(1, int(check_every))
        self.iterations_run = {}
        # Validation monitor (fit(..., validation=...)): per restart the held-out log-likelihood at every check as
        # [(iterations done, value), ...] and the iteration count of its best check, whose parameters `results` holds
        self.validation_curve = {}
        self.best_iteration = {}
        self._monitor = None     # (encoded validation rows, patience) while a monitored fit runs
        # src/mmsbm.py:81-85
        self.rng = np.random.default_rng(seed)
        self.child_states = self.rng.bit_generator._seed_seq.spawn(sampling)
        self.logger = logging.getLogger("MMSBM")
        self._backend = None  # resolved in _prepare_objects, like the reference (EM ctor)
        self.best_by_likelihood = None
        self._ctxs = {}
        self._resident = {}      # (device, context) -> restart ids whose final parameters sit in its slots
        self._scored = None      # (prediction matrix, raw device sums) of the last predict()

    # ------------------------------------------------------------------ preparation
    def _prepare_objects(self, train):
        """Dims only; the degrees come from the device layout (src/mmsbm.py:93-146 minus the
        dead O(U*N) index lists)."""
        # 'auto'/'hip' -> hip; anything else raises ImportError like src/backend.py:27-28
        *_, self._backend = load_backend(self.backend)
        train = np.asarray(train)
        self.train = train
        # = sorted(set(train[:, 2])), src/mmsbm.py:95 (ids are small non-negative ints: one counting pass)
        self.ratings = (np.flatnonzero(np.bincount(train[:, 2])).tolist() if len(train) else [])
        self.r = max(self.ratings)
        self.p = int(train[:, 0].max())
        self.m = int(train[:, 1].max())
        self._dims = {"n_samples": len(train), "n_user_groups": self.user_groups,
                      "n_item_groups": self.item_groups, "n_ratings": len(self.ratings)}
        self._release()

    def _device_list(self):
        if self.devices is not None:
            return list(dict.fromkeys(int(d) for d in self.devices))  # unique, order kept
        return [0]

    def _ctx(self, device, slot=0):
        ctx = self._ctxs.get((device, slot))
        if ctx is None:
            ctx = HipEM(self.train, self.user_groups, self.item_groups, n_users=self.p + 1,
                        n_items=self.m + 1, n_ratings=self._dims["n_ratings"], device=device)
            self._ctxs[(device, slot)] = ctx
        return ctx

    def _sharers(self, device):
        """Workers that may size a batch of restart slots on `device` at the same time."""
        lanes = list(self.devices) if self.devices is not None else [0]
        return max(1, self.contexts_per_device * max(1, sum(1 for d in lanes if int(d) == int(device))))

    def _release(self):
        for ctx in self._ctxs.values():
            ctx.close()
        self._ctxs = {}
        self._resident = {}

    # ------------------------------------------------------------------ training
    def fit(self, data, silent=False, validation=None, patience=None):
        """``validation``: rows the fit does not train on (same columns as ``data``; users, items and ratings unseen in
        ``data`` are dropped with ``predict``'s warning).  Every ``check_every`` iterations, and after the last one,
        the held-out log-likelihood sum log P(observed rating | user, item) of every restart is evaluated on the
        device; a restart's parameters at its best check (the first one with the highest value) are kept there and are
        what ``results`` holds -- with ``"likelihood"`` the training likelihood of exactly those parameters and
        ``"validation"`` the value at that check.  ``validation_curve[i]`` and ``best_iteration[i]`` record restart
        i's checks.  ``patience=p`` stops a batch of restarts after a check at which each of them has had p
        consecutive checks without a new best; None runs all iterations."""
        self._check_monitor_args(validation, patience)
        if not silent:
            self.logger.info(f"Running {self.sampling} runs of {self.iterations} iterations.")
        encoder = Encoder()
        train = encoder.fit_transform(data)
        if validation is not None:
            validation = encoder.transform(validation, self.logger)
            if len(validation) == 0:
                raise ValueError(self._NO_VALIDATION_ROW)
        self.data_handler = encoder   # (only now: a refused fit leaves a fitted model, its encoder included, as it was)
        self.fit_encoded(train, validation=validation, patience=patience)

    _NO_VALIDATION_ROW = ("the validation set has no row left after encoding: every row names a user, an item or a "
                          "rating that is not in the training data")

    def _check_monitor_args(self, validation, patience):
        """The refusals of a monitored fit that need no data (before anything is encoded or sent to a device)."""
        if patience is not None:
            if isinstance(patience, (bool, np.bool_)) or not isinstance(patience, (int, np.integer)) or patience < 1:
                raise ValueError(f"patience must be a positive integer, got {patience!r}")
            if validation is None:
                raise ValueError("patience needs a validation set: it counts checks without a new best on it")
        if validation is not None and self.tol is not None:
            raise ValueError("validation and tol are two stop rules with no defined way to combine them: "
                             "construct the model with tol=None to monitor a validation set")

    def fit_encoded(self, train, restarts=None, validation=None, patience=None):
        """fit() on already encoded (N,3) triples.  ``restarts``: subset of restart indices to
        run here (used by the multi-GPU driver); default all.  ``validation`` / ``patience``: as in ``fit``, encoded
        (M,3) triples; rows with an id outside the training ones are dropped with a warning."""
        self._check_monitor_args(validation, patience)
        if validation is not None:
            t = np.asarray(train)
            validation = self._known_rows(validation, int(t[:, 0].max()) + 1, int(t[:, 1].max()) + 1,
                                          np.flatnonzero(np.bincount(t[:, 2])))
            if len(validation) == 0:
                raise ValueError(self._NO_VALIDATION_ROW)
        self.validation_curve, self.best_iteration = {}, {}
        self._monitor = None if validation is None else (validation, None if patience is None else int(patience))
        try:
            return self._fit_prepared(train, restarts)
        finally:
            self._monitor = None

    def _fit_prepared(self, train, restarts):
        self._prepare_objects(train)
        todo = list(range(self.sampling)) if restarts is None else list(restarts)
        # workers = (GPU, context slot); restart j of `todo` goes to worker j mod #workers
        workers = [(d, s) for s in range(self.contexts_per_device) for d in self._device_list()]
        workers = workers[:max(1, len(todo))]

        def work(w):  # this worker's restarts, in batches of slots
            dev, slot = workers[w]
            mine, out = todo[w::len(workers)], []
            per = self.restarts_per_launch or self._ctx(dev, slot).suggested_slots()
            for b in range(0, len(mine), per):
                batch = mine[b:b + per]
                out.extend(zip(batch, self.run_samplings(batch, device=dev, slot=slot)))
            return out

        if len(workers) == 1:
            parts = [work(0)]
        else:  # one host thread per worker; ctypes releases the GIL inside the library
            with ThreadPoolExecutor(max_workers=len(workers)) as pool:
                parts = list(pool.map(work, range(len(workers))))
        by_i = dict(x for part in parts for x in part)
        done = [by_i[i] for i in todo]
        self.results = done
        self._restart_ids = todo
        liks = [float(r["likelihood"]) for r in done]
        self.best_by_likelihood = todo[int(np.argmax(liks))] if liks else None
        return self

    def init_params(self, seed, d_u, d_i):
        """theta0, eta0, p0 with the reference's draw order (src/mmsbm.py:224-233)."""
        rng = np.random.default_rng(seed)
        k, l, r = self.user_groups, self.item_groups, self._dims["n_ratings"]
        theta = rng.random((self.p + 1, k)) / d_u[:, None]
        eta = rng.random((self.m + 1, l)) / d_i[:, None]
        pr = normalize_with_self(rng.random((k, l, r)))
        return theta, eta, pr

    def run_samplings(self, ids, device=0, slot=0, seeds=None):
        """Restarts ``ids`` together, device resident, as the slots of one context
        (src/mmsbm.py:187-269 for each of them).  Returns their result dicts in order."""
        ctx = self._ctx(device, slot)
        ids = list(ids)
        seeds = [self.child_states[i] for i in ids] if seeds is None else list(seeds)
        if len(ids) > 1:
            # memory: what is FREE on the device now, shared with the other workers on this GPU
            fit_in = ctx.max_slots(0.5, sharers=self._sharers(device))
            if len(ids) > fit_in:  # run what fits, then the rest
                return (self.run_samplings(ids[:fit_in], device, slot, seeds[:fit_in]) +
                        self.run_samplings(ids[fit_in:], device, slot, seeds[fit_in:]))
        try:
            ctx.set_slots(len(ids))
        except HipLibraryError:
            # the device ran out of memory after all (another worker got there first): the
            # context is back to one slot; halve the batch and try again
            if len(ids) == 1:
                raise
            half = len(ids) // 2
            return (self.run_samplings(ids[:half], device, slot, seeds[:half]) +
                    self.run_samplings(ids[half:], device, slot, seeds[half:]))
        for s, seed in enumerate(seeds):  # theta0, eta0 are drawn on the device (same PCG64 stream)
            ctx.select(s).init_params(seed)
        if self._monitor is not None:
            # The snapshot tables -- a further theta + eta + p for every slot, which max_slots() does not count -- are
            # allocated by the first save: make it now, before any iteration, so that a batch they do not fit beside
            # is halved like one whose slots do not fit.  (The start it saves is replaced by the first check.)
            try:
                ctx.select(0).snapshot_save()
            except HipLibraryError:
                if len(ids) == 1:
                    raise
                half = len(ids) // 2
                return (self.run_samplings(ids[:half], device, slot, seeds[:half]) +
                        self.run_samplings(ids[half:], device, slot, seeds[half:]))
            out = self._run_monitored(ctx, ids)
            self._resident[(device, slot)] = ids
            return out
        done = 0
        if self.debug or self.tol is not None:
            # src/mmsbm.py:252-254 evaluates the likelihood inside the loop when j % 50 == 0, i.e.
            # after iterations 1, 51, 101, ...; the convergence monitor (tol) checks every
            # `check_every` iterations instead.
            last = None
            while done < self.iterations:
                if self.tol is None:
                    step = min(1 if done == 0 else 50, self.iterations - done)
                else:
                    step = min(self.check_every, self.iterations - done)
                ctx.iterate(step)
                done += step
                if self.tol is None and (done - 1) % 50 != 0:
                    break  # the tail after the last hook: the reference logs nothing there
                liks = np.array([ctx.select(s).likelihood() for s in range(len(ids))])
                if self.debug:
                    for i, lik in zip(ids, liks):
                        self.logger.debug(f"\nLikelihood at run {i} is {lik:.0f}")
                if self.tol is not None and last is not None and np.all(
                        np.abs(liks - last) <= self.tol * np.abs(last)):
                    break
                last = liks
        else:
            ctx.iterate(self.iterations)
            done = self.iterations
        for i in ids:
            self.iterations_run[i] = done
        out = []
        for s in range(len(ids)):
            likelihood, theta, eta, pr = ctx.select(s).result()
            out.append({"likelihood": likelihood, "pr": pr, "theta": theta, "eta": eta})
        self._resident[(device, slot)] = ids
        return out

    def _run_monitored(self, ctx, ids):
        """The iterations of the restarts in ctx's slots with the validation monitor of ``fit``: a check is ONE
        heldout_eval for the whole batch; a restart's new best (strictly greater: the first of equal values stays)
        saves its slot's parameters on the device.  Returns the result dicts of the kept parameters; the slots hold
        them afterwards."""
        validation, patience = self._monitor
        n = len(ids)
        best, best_it, stale = [None] * n, [0] * n, [0] * n
        curves = [[] for _ in range(n)]
        done = 0
        ctx.heldout_begin(validation)
        try:
            while True:
                step = min(self.check_every, self.iterations - done)
                if step > 0:
                    ctx.iterate(step)
                    done += step
                values = ctx.heldout_eval()
                for s in range(n):
                    v = float(values[s])
                    curves[s].append((done, v))
                    if best[s] is None or v > best[s]:
                        best[s], best_it[s], stale[s] = v, done, 0
                        ctx.select(s).snapshot_save()
                    else:
                        stale[s] += 1
                if self.debug:
                    for i, v in zip(ids, values):
                        self.logger.debug(f"\nHeld-out log-likelihood at run {i} after {done} iterations is {v:.0f}")
                if done >= self.iterations or (patience is not None and all(c >= patience for c in stale)):
                    break
        finally:
            ctx.heldout_end()
        out = []
        for s, i in enumerate(ids):
            self.iterations_run[i] = done
            self.validation_curve[i] = curves[s]
            self.best_iteration[i] = best_it[s]
            ctx.select(s)
            if best_it[s] != done:  # the kept parameters go back into the slot (through the host, once per restart)
                ctx.set_params(*ctx.snapshot_get())
            likelihood, theta, eta, pr = ctx.result()
            out.append({"likelihood": likelihood, "pr": pr, "theta": theta, "eta": eta, "validation": best[s]})
        return out

    def run_one_sampling(self, data, seed, i, device=0, slot=0):
        """One restart, device resident (src/mmsbm.py:187-269)."""
        return self.run_samplings([i], device, slot, seeds=[seed])[0]

    # ------------------------------------------------------------------ prediction
    def _check_is_fitted(self):
        assert self.results is not None, "You need to fit the model before predicting."

    def _check_has_predictions(self):
        assert self.prediction_matrix is not None, (
            "You need to predict before computing the goodness of fit parameters.")

    def predict(self, data):
        """Mean of prod_dist over restarts; stored objects from the run with the best test
        accuracy (src/mmsbm.py:279-317).  Everything per test row -- the distributions, their
        running sum over restarts, argmax and the indicators of src/mmsbm.py:488-528 -- is
        evaluated on the device; per restart only six sums come back."""
        self._check_is_fitted()
        if len(self._restart_ids) != self.sampling:
            # restarts.fit_distributed(gather=False) left this rank with ITS share only: a mean over that share
            # would silently differ from rank to rank (the reference averages over all restarts, src/mmsbm.py:315)
            raise RuntimeError(
                f"this model holds {len(self._restart_ids)} of its {self.sampling} restarts (restarts.fit_distributed "
                "without gather=True): use mmsbm_amd.restarts.predict_distributed(model, data), or fit with gather=True")
        test = self.data_handler.transform(data, self.logger)
        matrix, raw, per_run = self._predict_runs(test)
        self.run_stats = per_run
        self._keep_best_run(int(np.argmax([st["accuracy"] for st in per_run])))  # first best restart, src/mmsbm.py:474-478
        self.prediction_matrix = matrix
        self._scored = (matrix, raw)
        return self.prediction_matrix

    def _predict_runs(self, test, subset=None):
        """The restarts held by THIS model (all of them, or this rank's share) on encoded test triples:
        (mean distribution over them, its six sums, the five scores of every restart).  ``subset``:
        positions in ``self.results`` to score instead of all of them (restarts.predict_distributed)."""
        self.test = test
        ctx, restarts = self._restarts(subset)
        ctx.predict_begin(test, np.asarray(self.ratings, dtype=np.float64))
        per_run = [ctx.predict_add() for _ in restarts]
        matrix, raw = ctx.predict_finish()
        self._raw_per_run = per_run                  # the six sums of each scored restart (restarts.predict_distributed)
        return matrix, raw, [ctx.final_stats(st) for st in per_run]

    def _restarts(self, subset=None):
        """(ctx, restarts): this model's context on its first device, and an iterator over the positions ``subset`` in
        ``self.results`` (None: all of them) that selects each restart's parameters in the context before it yields
        the position.  Restarts whose final parameters still sit in the context's slots are selected there and need no
        upload; otherwise the context drops to one slot here and each restart is uploaded in its turn."""
        dev = self._device_list()[0]
        ctx = self._ctx(dev)
        picked = range(len(self.results)) if subset is None else list(subset)
        resident = self._resident.get((dev, 0)) == list(self._restart_ids) and ctx.slots == len(self.results)
        if not resident:
            ctx.set_slots(1)
            self._resident.pop((dev, 0), None)

        def each():
            for j in picked:
                if resident:
                    ctx.select(j)
                else:
                    a = self.results[j]
                    ctx.set_params(a["theta"], a["eta"], a["pr"])
                yield j
        return ctx, each()

    # ------------------------------------------------------------------ recommendation (not in the reference)
    RECOMMEND_BATCH_ROWS = 1 << 22   # result rows (users x n) fetched from the device per query call

    def recommend(self, users=None, n=10, exclude_seen=True, weights=None, candidates=None, exclude=None):
        """The ``n`` best items per user, scored on the device: score(u, i) = sum_r weights[r] P(r | u, i), mean over
        the restarts the model holds -- with the default weights (the rating values, ``self.ratings``) the expected
        rating that ``predict`` + ``score`` use.  Candidates are all training items, without the user's own training
        items when ``exclude_seen``.  Order: score descending, equal scores by ascending encoded item id.

        ``candidates``: an iterable of item labels -- the items in stock, of one category, released this week; only
        they are scored and ranked (duplicates count once; a label that is not in the training data: KeyError; an
        empty one: an empty frame).  ``exclude``: further (user, item) pairs to leave out -- shown, dismissed, bought
        elsewhere -- as a DataFrame whose first two columns are users and items or an iterable of (user, item) tuples;
        pairs of users that are not requested, and pairs with a user or an item that is not in the training data, are
        ignored.  Scores and order are those of the plain call: the answer is its list for n = all items, filtered.

        Returns a DataFrame with columns ``users``, ``items``, ``score``, ``rank`` (1 = best), users in request order
        (``users=None``: every training user), users and items as the encoder's labels (``theta`` / ``eta``'s index).  The model's stored predictions and
        ``score()`` are left as they are."""
        self._check_whole_model()
        n, w = self._recommend_args(n, weights)
        enc = self.data_handler
        ids, labels = self._training_users(users)
        item_labels = np.asarray(enc.item_labels(), dtype=object) if enc else None
        if candidates is None and exclude is None:
            with self._session_of_restarts("recommend", w, exclude_seen) as ctx:
                return self._top_n_frame(lambda b, e: ctx.recommend_query(ids[b:e], n), n, labels, item_labels)
        cand = None if candidates is None else self._candidate_ids(candidates)
        if cand is not None and len(cand) == 0:
            return self._top_n_frame(None, n, labels[:0], item_labels)
        off, its = (None, None) if exclude is None else self._exclusion_lists(exclude, ids)
        with self._session_of_restarts("recommend", w, exclude_seen) as ctx:
            def query(b, e):
                extra = None if off is None else (off[b:e + 1] - off[b], its[off[b]:off[e]])
                return ctx.recommend_query_within(ids[b:e], n, cand, extra)
            return self._top_n_frame(query, n, labels, item_labels)

    RECOMMEND_MAX = 1024             # largest n of a top-N query (MMSBM_HIP_RECOMMEND_MAX_N)

    def rerank(self, pairs, n=None, exclude_seen=True, weights=None):
        """The order of caller-given candidates per user -- the second stage of a two-stage system: a cheap retriever
        proposes a few hundred items per user, the model orders them.  ``pairs``: a DataFrame whose first two columns
        are users and items (further columns are ignored), or an iterable of (user, item) tuples; both must be in the
        training data (KeyError).  A user's candidates are the items of its pairs (a repeated pair counts once),
        without the user's own training items when ``exclude_seen``.  Scores and order are ``recommend``'s, bit for
        bit, and everything runs on the device.

        ``n``: the best ``n`` of each list; None: each user's whole list, provided the longest holds at most 1,024
        items (a longer one needs an explicit ``n``).  Returns ``recommend``'s frame (``users``, ``items``, ``score``,
        ``rank``), users in order of first appearance in ``pairs``.  The model's stored predictions and ``score()``
        are left as they are."""
        self._check_whole_model()
        w = self._rating_weights(weights)
        if n is not None:
            n, _ = self._recommend_args(n, weights)
        us, its = self._pair_columns(pairs)
        uid, _ = self._training_ids(us, "users")
        iid, _ = self._training_ids(its, "items")
        enc = self.data_handler
        item_labels = np.asarray(enc.item_labels(), dtype=object) if enc else None
        users, first = np.unique(uid, return_index=True)
        users = users[np.argsort(first, kind="stable")]                    # order of first appearance
        place = np.empty((self.p + 1), dtype=np.int64)
        place[users] = np.arange(len(users))
        rows = np.unique(np.stack([place[uid], iid.astype(np.int64)], 1), axis=0) if len(uid) else np.zeros((0, 2), np.int64)
        off = np.concatenate([[0], np.cumsum(np.bincount(rows[:, 0], minlength=len(users)))]).astype(np.int64)
        items = rows[:, 1].astype(np.int32)                                 # per user ascending and distinct
        users = users.astype(np.int32)
        labels = np.asarray(enc.user_labels(), dtype=object)[users] if enc else users
        if n is None:
            longest = int(np.diff(off).max()) if len(users) else 1
            if longest > self.RECOMMEND_MAX:
                raise ValueError(f"the longest candidate list holds {longest} items: beyond {self.RECOMMEND_MAX} "
                                 "an explicit n is needed")
            n = max(longest, 1)
        if len(users) == 0:
            return self._top_n_frame(None, n, labels[:0], item_labels)
        with self._session_of_restarts("recommend", w, exclude_seen) as ctx:
            return self._top_n_frame(
                lambda b, e: ctx.recommend_rank(users[b:e], off[b:e + 1] - off[b], items[off[b]:off[e]], n),
                n, labels, item_labels)

    def _candidate_ids(self, candidates):
        """The encoded ids of ``candidates`` (item labels of the training data: KeyError otherwise), ascending and
        distinct, int32."""
        return np.unique(self._training_ids(list(candidates), "items")[0]).astype(np.int32)

    @staticmethod
    def _pair_columns(pairs):
        """(users, items) of a ``pairs`` argument: the first two columns of a DataFrame, or (user, item) tuples."""
        if hasattr(pairs, "iloc") and hasattr(pairs, "columns"):
            if pairs.shape[1] < 2:
                raise ValueError("pairs needs two columns: users and items")
            return pairs.iloc[:, 0].tolist(), pairs.iloc[:, 1].tolist()
        rows = [tuple(x) for x in pairs]
        if any(len(x) != 2 for x in rows):
            raise ValueError("pairs must be (user, item) tuples")
        return [x[0] for x in rows], [x[1] for x in rows]

    def _exclusion_lists(self, exclude, ids):
        """(offsets (len(ids) + 1,) int64, items int32): for every requested row (encoded user ``ids``) the distinct
        encoded items ``exclude`` names for that user, ascending; pairs of other users and unknown labels are dropped."""
        us, its = self._pair_columns(exclude)
        uid, iid = self._lookup_ids(us, "users"), self._lookup_ids(its, "items")
        keep = (uid >= 0) & (iid >= 0) & np.isin(uid, ids)
        rows = np.unique(np.stack([uid[keep], iid[keep]], 1).astype(np.int64), axis=0) if keep.any() else np.zeros((0, 2), np.int64)
        start = np.searchsorted(rows[:, 0], ids, side="left")               # rows: by user, then item, both ascending
        stop = np.searchsorted(rows[:, 0], ids, side="right")
        off = np.concatenate([[0], np.cumsum(stop - start)]).astype(np.int64)
        pick = np.concatenate([np.arange(a, b) for a, b in zip(start.tolist(), stop.tolist())]) if len(ids) else []
        return off, rows[np.asarray(pick, dtype=np.int64), 1].astype(np.int32)

    def recommend_users(self, items=None, n=10, exclude_seen=True, weights=None):
        """The ``n`` best users per item -- who should see this item -- scored on the device: ``recommend`` from the
        item's side.  Scores as in ``recommend`` (the same numbers, bit for bit); candidates are all training users,
        without the users that have the item in the training data when ``exclude_seen``.  Order: score descending,
        equal scores by ascending encoded user id.

        Returns a DataFrame with columns ``items``, ``users``, ``score``, ``rank`` (1 = best), items in request order
        (``items=None``: every training item), labels as ``recommend`` returns them.  The model's stored predictions
        and ``score()`` are left as they are."""
        self._check_whole_model()
        n, w = self._recommend_args(n, weights)
        enc = self.data_handler
        ids, labels = self._training_ids(items, "items")
        user_labels = np.asarray(enc.user_labels(), dtype=object) if enc else None
        with self._session_of_restarts("recommend", w, exclude_seen) as ctx:
            return self._top_n_frame(lambda b, e: ctx.recommend_query_items(ids[b:e], n), n, labels, user_labels,
                                     columns=("items", "users", "score"))

    def audience(self, items=None, min_score=None, exclude_seen=True, weights=None, count_only=False):
        """Every user whose score for an item reaches ``min_score`` (required, finite) -- a mailing list, the reach of a
        campaign -- found on the device without a users x items score matrix.  Scores and candidates as in
        ``recommend_users``; the bar is compared with the final score.

        Returns a DataFrame with columns ``items``, ``users``, ``score``, ``rank`` (1 = the item's best user): items in
        request order (``items=None``: every training item), within an item score descending, equal scores by
        ascending encoded user id.  ``count_only=True``: columns ``items``, ``count``, one row per requested item.  The
        model's stored predictions and ``score()`` are left as they are."""
        import pandas as pd
        self._check_whole_model()
        if (isinstance(min_score, (bool, np.bool_)) or not isinstance(min_score, (int, float, np.integer, np.floating))
                or not np.isfinite(min_score)):
            raise ValueError(f"min_score must be a finite number, got {min_score!r}")
        min_score, w = float(min_score), self._rating_weights(weights)
        enc = self.data_handler
        ids, labels = self._training_ids(items, "items")
        user_labels = np.asarray(enc.user_labels(), dtype=object) if enc else None
        with self._session_of_restarts("recommend", w, exclude_seen) as ctx:
            sizes = np.diff(ctx.recommend_audience(ids, min_score, count_only=True)[0])
            if count_only:
                return pd.DataFrame({"items": labels, "count": sizes.astype(np.int64)})
            parts = []
            b = 0
            while b < len(ids):  # pieces of at most RECOMMEND_BATCH_ROWS entries (a larger item goes alone)
                e, total = b + 1, int(sizes[b])
                while e < len(ids) and total + int(sizes[e]) <= self.RECOMMEND_BATCH_ROWS:
                    total += int(sizes[e])
                    e += 1
                off, us, sc = ctx.recommend_audience(ids[b:e], min_score, total=total)
                at = np.repeat(np.arange(b, e), np.diff(off))
                order = np.lexsort((us, -sc, at))
                us, sc, at = us[order], sc[order], at[order]
                parts.append(pd.DataFrame({
                    "items": labels[at] if len(at) else np.empty(0, dtype=object),
                    "users": user_labels[us] if user_labels is not None else us.astype(np.int64),
                    "score": sc,
                    "rank": (np.arange(len(at)) - off[:-1][at - b] + 1).astype(np.int64)}))
                b = e
        if not parts:
            return pd.DataFrame({"items": [], "users": [], "score": np.zeros(0), "rank": np.zeros(0, dtype=np.int64)})
        return pd.concat(parts, ignore_index=True)

    TOP_PAIRS_MAX = 1024             # largest m of top_pairs (MMSBM_HIP_TOP_PAIRS_MAX_M)

    def top_pairs(self, m=100, users=None, exclude_seen=True, weights=None):
        """The ``m`` best (user, item) pairs of the whole model, ranked on the device in ONE order over all pairs of
        ``users`` (None: every training user) and the training items -- the most probable missing links of a network,
        the strongest matches of a catalogue.  Scores as in ``recommend`` (the same numbers, bit for bit); candidates
        are all pairs, without the training pairs when ``exclude_seen``.  Order: score descending, equal scores by
        ascending encoded user id, then encoded item id; the order in which ``users`` are named does not matter.

        Returns a DataFrame with columns ``users``, ``items``, ``score``, ``rank`` (1 = best of all), at most ``m``
        rows, labels as ``recommend`` returns them.  The model's stored predictions and ``score()`` are left as they
        are."""
        import pandas as pd
        self._check_whole_model()
        if isinstance(m, (bool, np.bool_)) or not isinstance(m, (int, np.integer)) or m < 1:
            raise ValueError(f"m must be a positive integer, got {m!r}")
        if m > self.TOP_PAIRS_MAX:
            raise ValueError(f"m = {m} is beyond the {self.TOP_PAIRS_MAX} pairs a query returns at most")
        m, w = int(m), self._rating_weights(weights)
        enc = self.data_handler
        ids = None
        if users is not None:
            ids, labels = self._training_users(users)
            if len(np.unique(ids)) != len(ids):
                twice = list(dict.fromkeys(labels[np.isin(ids, ids[np.bincount(ids)[ids] > 1])].tolist()))
                raise ValueError(f"users named more than once: {twice}")
        with self._session_of_restarts("recommend", w, exclude_seen) as ctx:
            us, its, scores, count = ctx.recommend_top_pairs(m, ids)
        us, its = us[:count].astype(np.int64), its[:count].astype(np.int64)
        return pd.DataFrame({
            "users": np.asarray(enc.user_labels(), dtype=object)[us] if enc else us,
            "items": np.asarray(enc.item_labels(), dtype=object)[its] if enc else its,
            "score": scores[:count],
            "rank": np.arange(1, count + 1, dtype=np.int64)})

    def explain(self, pairs, n=5, weights=None):
        """Why an item is recommended to a user: the ``n`` training rows of the user that carry most of the pair's
        score -- the "because you rated ..." of a recommendation -- found on the device.

        With eta and p fixed, the theta half of the M-step writes a user's membership as an average over the user's
        d_u training rows j = (u, i_j, r_j): theta'_u[k] = (1/d_u) sum_j c_j[k], where c_j[k] = theta_u[k] v_j[k] /
        (theta_u . v_j) is the share of row j that group k takes and v_j[k] = sum_l p[k, l, r_j] eta[i_j, l].  The score
        is linear in theta, score(u, t) = sum_k theta_u[k] g_t[k] with g_t[k] = sum_l (sum_r weights[r] p[k, l, r])
        eta[t, l], so contribution(u, t, j) = (1/d_u) sum_k c_j[k] g_t[k] is the part of the score that row j carries
        (d_u times it: the score u would have for t if judged from row j alone).  The contributions of ALL the user's
        rows, not only the ``n`` returned, sum to ``explained``, the score under one more theta update; ``explained``
        equals ``score`` at a fixed point of EM, so ``score - explained`` is how far that user's theta is from one.
        Everything is the mean over the restarts the model holds.

        ``pairs``: a DataFrame whose first two columns are users and items (further columns are ignored, so
        ``model.explain(model.recommend(users=[...]))`` works as is), or an iterable of (user, item) tuples; both must
        be in the training data (KeyError).  Returns a DataFrame with columns ``users``, ``items``, ``because`` (the
        history item), ``rating`` (the rating the user gave it), ``contribution``, ``share`` (contribution /
        explained), ``rank`` (1 = the largest contribution), ``score``, ``explained`` (both repeated on a pair's rows):
        pairs in request order, labels as ``recommend`` returns them; within a pair contribution descending, equal
        ones by ascending encoded history item id, then rating id.  The model's stored predictions and ``score()`` are
        left as they are."""
        import pandas as pd
        self._check_whole_model()
        n, w = self._recommend_args(n, weights)
        us, its = self._pair_columns(pairs)
        uid, ulab = self._training_ids(us, "users")
        iid, ilab = self._training_ids(its, "items")
        enc = self.data_handler
        item_labels = np.asarray(enc.item_labels(), dtype=object) if enc else None
        rating_labels = np.asarray(enc.rating_labels(), dtype=object) if enc else None
        q_all = len(uid)
        step = max(1, self.RECOMMEND_BATCH_ROWS // n)
        parts = []
        with self._session_of_restarts("explain", w) as ctx:
            for b in range(0, q_all, step):
                e = min(q_all, b + step)
                u = uid[b:e]
                first = np.flatnonzero(np.concatenate([[True], u[1:] != u[:-1]]))   # runs of one user: one occurrence
                off = np.concatenate([first, [e - b]]).astype(np.int64)
                hi, hr, co, counts, explained, score, _ = ctx.explain_query(u[first], off, iid[b:e], n)
                keep = np.arange(n)[None, :] < counts[:, None]
                at = np.repeat(np.arange(b, e), counts)
                it, rt, cv = hi[keep], hr[keep], co[keep]
                ex = explained[at - b]
                parts.append(pd.DataFrame({
                    "users": ulab[at] if len(at) else np.empty(0, dtype=object),
                    "items": ilab[at] if len(at) else np.empty(0, dtype=object),
                    "because": item_labels[it] if item_labels is not None else it.astype(np.int64),
                    "rating": rating_labels[rt] if rating_labels is not None else rt.astype(np.int64),
                    "contribution": cv,
                    "share": cv / ex,
                    "rank": np.nonzero(keep)[1].astype(np.int64) + 1,
                    "score": score[at - b],
                    "explained": ex}))
        if not parts:
            return pd.DataFrame({"users": [], "items": [], "because": [], "rating": [], "contribution": np.zeros(0),
                                 "share": np.zeros(0), "rank": np.zeros(0, dtype=np.int64), "score": np.zeros(0),
                                 "explained": np.zeros(0)})
        return pd.concat(parts, ignore_index=True)

    @staticmethod
    @contextlib.contextmanager
    def _recommend_session(ctx, weights, exclude_seen):
        """ctx's recommend session around the block, ended however the block ends."""
        ctx.recommend_begin(weights, exclude_seen)
        try:
            yield
        finally:
            ctx.recommend_end()

    @contextlib.contextmanager
    def _session_of_restarts(self, kind, *begin_args):
        """The context, with its ``kind`` session ("recommend", "similar", "overlap", "explain") begun with ``begin_args`` and
        every restart the model holds added to it, around the block; the session is ended however the block ends."""
        ctx, restarts = self._restarts()
        getattr(ctx, kind + "_begin")(*begin_args)
        try:
            for _ in restarts:
                getattr(ctx, kind + "_add")()
            yield ctx
        finally:
            getattr(ctx, kind + "_end")()

    @contextlib.contextmanager
    def _sessions_of_restarts(self, *sessions):
        """_session_of_restarts for several kinds at once: ``sessions`` are (kind, *begin_args); every restart the model
        holds is selected ONCE and added to each of them in that order, so they hold the same slots in the same order.
        Every session begun is ended however the block ends."""
        ctx, restarts = self._restarts()
        with contextlib.ExitStack() as stack:
            for kind, *begin_args in sessions:
                getattr(ctx, kind + "_begin")(*begin_args)
                stack.callback(getattr(ctx, kind + "_end"))
            for _ in restarts:
                for kind, *_args in sessions:
                    getattr(ctx, kind + "_add")()
            yield ctx

    def _top_n_frame(self, query, n, row_labels, item_labels, columns=("users", "items", "score")):
        """The top-``n`` frame (users, items, score, rank) of rows [0, len(row_labels)), fetched in calls of at most
        RECOMMEND_BATCH_ROWS result rows (bounded host memory at a million users): ``query(b, e)`` -> (items, scores,
        counts) of rows [b, e).  ``item_labels``: the label of each item id, or None (the ids themselves).
        ``columns``: the names of the row, the returned-id and the value column (similar_items / similar_users)."""
        import pandas as pd
        rows_col, ids_col, value_col = columns
        n_rows = len(row_labels)
        step = max(1, self.RECOMMEND_BATCH_ROWS // n)
        parts = []
        for b in range(0, n_rows, step):
            items, scores, counts = query(b, min(n_rows, b + step))
            keep = np.arange(n)[None, :] < counts[:, None]
            at = np.repeat(np.arange(b, b + len(counts)), counts)
            it = items[keep]
            parts.append(pd.DataFrame({
                rows_col: row_labels[at] if len(at) else np.empty(0, dtype=object),
                ids_col: item_labels[it] if item_labels is not None else it.astype(np.int64),
                value_col: scores[keep],
                "rank": np.nonzero(keep)[1].astype(np.int64) + 1}))
        if not parts:
            return pd.DataFrame({rows_col: [], ids_col: [], value_col: np.zeros(0), "rank": np.zeros(0, dtype=np.int64)})
        return pd.concat(parts, ignore_index=True)

    def _training_users(self, users):
        """(encoded ids int32, labels) of recommend's ``users`` argument (None: every training user)."""
        return self._training_ids(users, "users")

    def _training_ids(self, wanted, side):
        """(encoded ids int32, labels) of a request for training users or items (``side``; None: all of them)."""
        enc = self.data_handler
        n_side = (self.p if side == "users" else self.m) + 1
        side_labels = (lambda: enc.user_labels()) if side == "users" else (lambda: enc.item_labels())
        if wanted is None:
            ids = np.arange(n_side, dtype=np.int32)
            labels = np.asarray(side_labels(), dtype=object) if enc else ids
        else:
            labels = np.asarray(list(wanted), dtype=object)
            ids = self._lookup_ids(labels, side)
            if (ids < 0).any():
                missing = list(dict.fromkeys(labels[ids < 0].tolist()))
                raise KeyError(f"{side} not in the training data: {missing}")
            if enc:  # the encoder's labels, as with None (7 and "7" are one user; the frames join on this column)
                labels = np.asarray(side_labels(), dtype=object)[ids]
        return ids, labels

    def _lookup_ids(self, labels, side):
        """The encoded id (int32) of every label of ``side`` ("users" / "items"), -1 where the training data has none."""
        enc = self.data_handler
        if enc:
            index = {lab: j for j, lab in enumerate(enc.user_labels() if side == "users" else enc.item_labels())}
            found = [index.get(str(x), -1) for x in labels]
        else:
            n_side = (self.p if side == "users" else self.m) + 1
            found = [int(x) if isinstance(x, (int, np.integer)) and 0 <= int(x) < n_side else -1 for x in labels]
        return np.asarray(found, dtype=np.int32)

    def _check_whole_model(self):
        self._check_is_fitted()
        if len(self._restart_ids) != self.sampling:
            raise RuntimeError(
                f"this model holds {len(self._restart_ids)} of its {self.sampling} restarts (restarts.fit_distributed "
                "without gather=True): fit with gather=True to recommend from all of them")

    def _recommend_args(self, n, weights):
        if isinstance(n, (bool, np.bool_)) or not isinstance(n, (int, np.integer)) or n < 1:
            raise ValueError(f"n must be a positive integer, got {n!r}")
        return int(n), self._rating_weights(weights)

    def _rating_weights(self, weights):
        w = np.asarray(self.ratings if weights is None else weights, dtype=np.float64)
        if w.shape != (len(self.ratings),):
            raise ValueError(f"weights has shape {w.shape}, expected ({len(self.ratings)},): one per rating value")
        if not np.isfinite(w).all():
            raise ValueError(f"weights must be finite, got {w.tolist()}")
        return w

    # ------------------------------------------------------------------ nearest items / users (not in the reference)
    def similar_items(self, items=None, n=10):
        """The ``n`` training items most similar to each of ``items`` (None: every training item), on the device.

        An item's rating profile is the rating distribution a member of each user group gives it,
        q[i, k, :] = sum_l eta[i, l] p[k, l, :]; the distance of two items is
        D(i, j) = sum_k m[k] |q[i, k, :] - q[j, k, :]|^2 / U with m[k] = sum_u theta[u, k] the users in group k: how
        differently a user drawn from the training population rates the two, in [0, 2], mean over the restarts the
        model holds.  It does not depend on how a restart happens to label its groups.

        Returns a DataFrame with columns ``items``, ``similar``, ``distance``, ``rank`` (1 = nearest), rows in request
        order, both id columns as the encoder's labels (``eta``'s index).  Order: distance ascending, equal distances
        by ascending encoded id; an item is never its own neighbour.  The model's stored predictions and ``score()``
        are left as they are."""
        return self._similar("items", items, n)

    def similar_users(self, users=None, n=10):
        """The ``n`` training users most similar to each of ``users`` (None: every training user): ``similar_items``
        with the sides exchanged -- q[u, l, :] = sum_k theta[u, k] p[k, l, :], weighted by the items in each item
        group.  Columns ``users``, ``similar``, ``distance``, ``rank``."""
        return self._similar("users", users, n)

    def _similar(self, side, wanted, n):
        self._check_whole_model()
        n, _ = self._recommend_args(n, None)
        ids, labels = self._training_ids(wanted, side)
        enc = self.data_handler
        side_labels = np.asarray(enc.user_labels() if side == "users" else enc.item_labels(), dtype=object) if enc else None
        with self._session_of_restarts("similar", side) as ctx:
            return self._top_n_frame(lambda b, e: ctx.similar_query(ids[b:e], n), n, labels, side_labels,
                                     columns=(side, "similar", "distance"))

    # ------------------------------------------------------------------ diversified lists (not in the reference)
    DIVERSE_POOL_MAX = 1024          # largest pool of a diversified query (MMSBM_HIP_RECOMMEND_MAX_N)

    def recommend_diverse(self, users=None, n=10, diversity=..., pool=None, exclude_seen=True, weights=None,
                          candidates=None, exclude=None):
        """``recommend`` re-ranked for diversity, on the device: a fitted model puts whole blocks of items on the same
        memberships, so a user's ``n`` best items are often near-copies of each other.  From the user's ``pool`` best
        candidates -- ``recommend(n=pool)``'s list, with the same ``exclude_seen``, ``weights``, ``candidates`` and
        ``exclude`` -- the best one is taken first; then, ``n - 1`` times, the candidate with the largest
        score + ``diversity`` x (distance to the nearest item taken so far), equal values to the better item of
        ``recommend``'s order.  The distance is ``similar_items``'s (``distances``).

        ``diversity`` is required: it is in score units per unit of distance, so no default fits every weighting.
        It must be finite and >= 0; 0 gives ``recommend(n)``'s list, and the larger it is the further apart the items
        of a list lie.  ``pool``: None means min(1024, 10 n); at least ``n`` and at most 1,024.

        Returns ``recommend``'s frame plus ``distance`` -- to the nearest item ranked above it in the list, +inf at
        rank 1: columns ``users``, ``items``, ``score``, ``distance``, ``rank``.  ``list_diversity`` summarises a
        list.  The model's stored predictions and ``score()`` are left as they are."""
        self._check_whole_model()
        n, w = self._recommend_args(n, weights)
        if diversity is ...:
            raise TypeError("recommend_diverse() needs diversity=: score units per unit of distance (0: plain recommend)")
        if isinstance(diversity, (bool, np.bool_)) or not isinstance(diversity, (int, float, np.integer, np.floating)) \
                or not np.isfinite(diversity) or diversity < 0:
            raise ValueError(f"diversity must be a finite number >= 0, got {diversity!r}")
        if pool is None:
            pool = min(self.DIVERSE_POOL_MAX, 10 * n)
        if isinstance(pool, (bool, np.bool_)) or not isinstance(pool, (int, np.integer)) or pool < 1:
            raise ValueError(f"pool must be a positive integer, got {pool!r}")
        if not n <= pool <= self.DIVERSE_POOL_MAX:
            raise ValueError(f"pool must lie in [n, {self.DIVERSE_POOL_MAX}], got pool={pool} with n={n}")
        pool, lam = int(pool), float(diversity)
        enc = self.data_handler
        ids, labels = self._training_users(users)
        item_labels = np.asarray(enc.item_labels(), dtype=object) if enc else None
        cand = None if candidates is None else self._candidate_ids(candidates)
        dist = []                                                           # the distance column, call by call

        def framed(query, row_labels):
            df = self._top_n_frame(query, n, row_labels, item_labels)
            df.insert(3, "distance", np.concatenate(dist) if dist else np.zeros(0))
            return df
        if cand is not None and len(cand) == 0:
            return framed(None, labels[:0])
        off, its = (None, None) if exclude is None else self._exclusion_lists(exclude, ids)
        with self._sessions_of_restarts(("recommend", w, exclude_seen), ("similar", "items")) as ctx:
            def query(b, e):
                extra = None if off is None else (off[b:e + 1] - off[b], its[off[b]:off[e]])
                items, scores, distances, counts = ctx.recommend_diverse(ids[b:e], n, pool, lam, cand, extra)
                dist.append(distances[np.arange(n)[None, :] < counts[:, None]])
                return items, scores, counts
            return framed(query, labels)

    def distances(self, pairs, side="items"):
        """The distance of given pairs of training items (``side="users"``: of training users), on the device:
        ``similar_items``'s D, the number ``recommend_diverse`` trades against the score.  ``pairs``: a DataFrame whose
        first two columns hold the two labels of each pair, or an iterable of 2-tuples; a label that is not in the
        training data: KeyError.  D(a, b) = D(b, a) bit for bit and D(a, a) = 0.

        Returns a DataFrame with columns ``a``, ``b`` (the encoder's labels), ``distance``, rows in request order."""
        import pandas as pd
        self._check_whole_model()
        if side not in ("items", "users"):
            raise ValueError(f"side must be 'items' or 'users', got {side!r}")
        left, right = self._pair_columns(pairs)
        a, a_labels = self._training_ids(left, side)
        b, b_labels = self._training_ids(right, side)
        if len(a) == 0:
            return pd.DataFrame({"a": [], "b": [], "distance": np.zeros(0)})
        with self._session_of_restarts("similar", side) as ctx:
            d = self._pair_distances(ctx, a, b)
        return pd.DataFrame({"a": a_labels, "b": b_labels, "distance": d})

    def _pair_distances(self, ctx, a, b):
        """ctx.similar_pairs in calls of at most RECOMMEND_BATCH_ROWS pairs."""
        step = self.RECOMMEND_BATCH_ROWS
        parts = [ctx.similar_pairs(a[s:s + step], b[s:s + step]) for s in range(0, len(a), step)]
        return np.concatenate(parts) if parts else np.zeros(0)

    def list_diversity(self, recs):
        """The intra-list distance of every user's list in a recommend-style frame (``recommend``,
        ``recommend_diverse``, ``rerank`` ...: the first two columns are users and items): the mean of ``distances``
        over the unordered pairs of the list's items, on the device -- what ``diversity=`` bought, to be read next to
        ``ranking_score``.  The items must be in the training data (KeyError); the users are only the lists' names.

        Returns a DataFrame with columns ``users`` (order of first appearance), ``n`` (items in the list) and
        ``diversity`` (NaN for a list of fewer than two items)."""
        import pandas as pd
        self._check_whole_model()
        us, its = self._pair_columns(recs)
        iid, _ = self._training_ids(its, "items")
        names = list(dict.fromkeys(us))
        place = {u: j for j, u in enumerate(names)}
        row = np.asarray([place[u] for u in us], dtype=np.int64)
        order = np.argsort(row, kind="stable")                             # each list's items, in the frame's order
        sizes = np.bincount(row, minlength=len(names))
        start = np.concatenate([[0], np.cumsum(sizes)])
        a, b, owner = [], [], []
        for j, k in enumerate(sizes.tolist()):
            if k >= 2:
                x, y = np.triu_indices(k, 1)
                mine = iid[order[start[j]:start[j + 1]]]
                a.append(mine[x])
                b.append(mine[y])
                owner.append(np.full(len(x), j, dtype=np.int64))
        total = np.zeros(len(names))
        if a:
            with self._session_of_restarts("similar", "items") as ctx:
                d = self._pair_distances(ctx, np.concatenate(a).astype(np.int32), np.concatenate(b).astype(np.int32))
            total = np.bincount(np.concatenate(owner), weights=d, minlength=len(names))
        pairs = sizes * (sizes - 1) // 2
        with np.errstate(divide="ignore", invalid="ignore"):
            mean = np.where(pairs > 0, total / np.maximum(pairs, 1), np.nan)
        return pd.DataFrame({"users": np.asarray(names, dtype=object) if names else [], "n": sizes.astype(np.int64),
                             "diversity": mean})

    # ------------------------------------------------------------------ matching the restarts' groups (not in the reference)
    def align_restarts(self, reference=None):
        """Which group of each restart is which group of restart ``reference``, and how well the restarts agree.

        Every restart labels its groups in an order of its own.  The overlap of two groups is the population they
        share, O[a, b] = sum_u theta_s[u, a] theta_t[u, b] (items: eta); the device computes it for all pairs of
        restarts at once, and each restart's groups are matched to the reference's by the assignment of the largest
        total overlap.  ``reference``: a position in ``self.results``; None: the restart of the highest training
        likelihood (the first of them).

        Returns a dict:
          ``reference``        the position used;
          ``user_groups``      (S, K) int64, ``[s, k]`` = the group of restart s matched to group k of the reference
                               (the identity for the reference itself);  ``item_groups`` (S, L) likewise;
          ``user_similarity``  (S, K), the cosine of each matched pair of theta columns, in [0, 1], 1 for the
                               reference; a column near 0 across the restarts is a group they do not reproduce -- the
                               usual sign of too large a K.  ``item_similarity`` (S, L) likewise;
          ``user_agreement``   (S, S), the largest assignment total of restarts s and t divided by the number of
                               users: the expected share of users the two put into matched groups; symmetric.
                               ``item_agreement`` likewise.
        ``self.results``, the stored predictions and ``score()`` are left as they are."""
        from . import align
        self._check_whole_model()
        S = len(self.results)
        if reference is None:
            reference = int(np.argmax([float(a["likelihood"]) for a in self.results]))   # (the first of the highest)
        elif isinstance(reference, (bool, np.bool_)) or not isinstance(reference, (int, np.integer)):
            raise ValueError(f"reference must be a position in self.results (an int) or None, got {reference!r}")
        elif not 0 <= reference < S:
            raise ValueError(f"reference = {reference} is not a position in self.results (0 .. {S - 1})")
        reference = int(reference)
        out = {"reference": reference}
        for side, groups, n_rows in (("user", self.user_groups, self.p + 1), ("item", self.item_groups, self.m + 1)):
            with self._session_of_restarts("overlap", side + "s") as ctx:
                gram = ctx.overlap_query()
            out[side + "_groups"], out[side + "_similarity"], out[side + "_agreement"] = align.align_side(
                gram, groups, n_rows, reference)
        return out

    def consensus(self, reference=None):
        """theta, eta and pr averaged over the restarts once their groups are matched (``align_restarts``).

        This is a DESCRIPTIVE summary, written in the group labels of restart ``reference`` (None: the restart of the
        highest training likelihood): what the restarts say about the groups on average, for reading memberships and
        judging which groups are reproducible.  It is not what the model predicts with: the predictive ensemble remains
        the mean over the restarts' own predictions that ``predict`` and ``recommend`` use, which needs no matching.

        Returns {"theta": DataFrame (user labels x K), "eta": DataFrame (item labels x L), "pr": {rating label: K x L
        DataFrame} (shaped as ``self.theta`` / ``self.eta`` / ``self.pr``), "alignment": the dict of
        ``align_restarts``}.  ``self.results`` and the stored objects are left as they are."""
        import pandas as pd
        from . import align
        alignment = self.align_restarts(reference)
        theta, eta, pr = align.consensus_params(self.results, alignment["user_groups"], alignment["item_groups"])
        enc = self.data_handler
        labels = enc.rating_labels() if enc else range(pr.shape[2])
        return {"theta": pd.DataFrame(theta, index=enc.user_labels() if enc else None),
                "eta": pd.DataFrame(eta, index=enc.item_labels() if enc else None),
                "pr": {lab: pd.DataFrame(pr[:, :, j]) for j, lab in enumerate(labels)},
                "alignment": alignment}

    # ------------------------------------------------------------------ ranking evaluation (not in the reference)
    def log_likelihood(self, data):
        """The held-out predictive log-likelihood of ``data`` (same columns as the training data), on the device:
        sum over the rows of log max(P(observed rating | user, item), eps) -- the quantity a probabilistic model is
        judged by, where ``score()`` reports the accuracy of the argmax.  Rows with a user, item or rating unseen in
        training are dropped with ``predict``'s warning.

        Returns {"rows": rows scored, "log_likelihood": that of the model's predictive distribution, the mean over the
        restarts as ``predict`` uses it, "per_restart": [that of each restart alone], "perplexity":
        exp(-log_likelihood / rows)}.  The model's stored predictions and ``score()`` are left as they are."""
        self._check_whole_model()
        rows = self._encode_heldout(data)
        ctx, restarts = self._restarts()
        ctx.heldout_begin(rows)
        try:
            per_restart = [float(ctx.heldout_add()) for _ in restarts]
            _, mean = ctx.heldout_mean(want_rows=False)
        finally:
            ctx.heldout_end()
        n, mean = len(rows), float(mean)
        return {"rows": n, "log_likelihood": mean, "per_restart": per_restart,
                "perplexity": float(np.exp(-mean / n)) if n else float("nan")}

    def _encode_heldout(self, data):
        """Encoded (N, 3) int32 rows of ``data`` in input order, rows with a user, item or rating unseen in training
        dropped with ``Encoder.transform``'s warning (after ``fit_encoded``: ids outside the training ones)."""
        if self.data_handler:
            return self.data_handler.transform(data, self.logger)
        return self._known_rows(data, self.p + 1, self.m + 1, self.ratings)

    def _known_rows(self, data, n_users, n_items, ratings):
        """The rows of encoded ``data`` whose ids are training ones (users below n_users, items below n_items, ratings
        among ``ratings``), (N, 3) int32 in input order; the others are dropped with ``Encoder.transform``'s warning."""
        from .encode import _columns
        cols, _ = _columns(data)
        keep = np.ones(len(cols[0]), dtype=bool)
        ids = []
        for name, col, known in (("users", cols[0], np.arange(n_users)), ("items", cols[1], np.arange(n_items)),
                                 ("ratings", cols[2], np.asarray(ratings))):
            col = np.asarray(col)
            if len(col) and not np.issubdtype(col.dtype, np.integer):
                raise ValueError(f"after fit_encoded the {name} column holds encoded integer ids")
            hit = np.isin(col, known)
            unseen = np.unique(col[keep & ~hit])
            if len(unseen):
                self.logger.warning(f"The {name} {', '.join(str(v) for v in unseen.tolist())} are in the test set "
                                    f"but weren't in the train set so I'll remove them.")
            keep &= hit
            ids.append(col)
        out = np.empty((int(keep.sum()), 3), dtype=np.int32)
        for j in range(3):
            out[:, j] = ids[j][keep]
        return out

    def _heldout(self, data, exclude_seen, weights):
        """(encoded rows (N, 3), position (N,), candidates (N,)) of every row of ``data`` that survives encoding."""
        self._check_whole_model()
        w = self._rating_weights(weights)
        rows = self._encode_heldout(data)
        users = rows[:, 0]
        order = np.argsort(users, kind="stable")                      # one request entry per user holding rows
        uniq, counts = np.unique(users[order], return_counts=True)
        offsets = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
        with self._session_of_restarts("recommend", w, exclude_seen) as ctx:
            pos, cand = ctx.recommend_positions(uniq.astype(np.int32), offsets, rows[order, 1])
        position = np.empty(len(rows), dtype=np.int64)
        position[order] = pos
        candidates = np.empty(len(rows), dtype=np.int64)
        candidates[order] = np.repeat(cand.astype(np.int64), counts)
        return rows, position, candidates

    def heldout_positions(self, data, exclude_seen=True, weights=None):
        """Where each held-out row's item falls in its user's full recommendation order, on the device: one row per
        row of ``data`` that survives encoding (rows whose user, item or rating is not in the training data are dropped
        with ``predict``'s warning), in input order.  Scores and candidates are those of ``recommend(users, n,
        exclude_seen, weights)``; ``position`` = 1 + the candidates that come before the item (score descending, equal
        scores by ascending encoded item id), 0 when the item is not a candidate (a training item of the user while
        ``exclude_seen``); ``candidates`` = the user's number of candidates.

        Returns a DataFrame with columns ``users``, ``items``, ``ratings`` (the encoder's labels), ``position`` and
        ``candidates``.  The model's stored objects are left as they are."""
        import pandas as pd
        rows, position, candidates = self._heldout(data, exclude_seen, weights)
        enc = self.data_handler
        cols = {}
        for j, name in enumerate(("users", "items", "ratings")):
            if enc:
                cols[name] = np.asarray(enc.labels[j], dtype=object)[rows[:, j]] if len(rows) else np.empty(0, dtype=object)
            else:
                cols[name] = rows[:, j].astype(np.int64)
        return pd.DataFrame({**cols, "position": position, "candidates": candidates})

    def _ranking_args(self, k, relevant):
        ks = [k] if isinstance(k, (int, np.integer)) and not isinstance(k, (bool, np.bool_)) else k
        if isinstance(ks, (str, bytes)) or not hasattr(ks, "__iter__"):
            raise ValueError(f"k must be a positive integer or a list of them, got {k!r}")
        ks = list(ks)
        if not ks or any(isinstance(x, (bool, np.bool_)) or not isinstance(x, (int, np.integer)) or x < 1 for x in ks):
            raise ValueError(f"k must be a positive integer or a list of them, got {k!r}")
        ks = list(dict.fromkeys(int(x) for x in ks))
        if relevant is None:
            return ks, None
        if isinstance(relevant, (str, bytes)) or not hasattr(relevant, "__iter__"):
            raise ValueError(f"relevant must be a collection of rating values, got {relevant!r}")
        enc = self.data_handler
        index = {lab: j for j, lab in enumerate(enc.rating_labels())} if enc else None
        ids = set()
        for v in relevant:
            if enc:  # the encoder's labels: str(value), whatever the order of the labels
                j = index.get(str(v), -1)
            else:
                j = int(v) if isinstance(v, (int, np.integer)) and int(v) in self.ratings else -1
            if j < 0:
                raise ValueError(f"relevant rating {v!r} is not a rating of the training data")
            ids.add(j)
        return ks, ids

    def ranking_score(self, data, k=10, relevant=None, exclude_seen=True, weights=None):
        """Top-N ranking metrics of the held-out rows ``data`` (users, items, ratings like ``predict``'s), from
        ``heldout_positions(data, exclude_seen, weights)``.  Each distinct (user, item) pair counts once; it is
        relevant when any of its rows has a rating in ``relevant`` (rating values as in the data, e.g. ``{4, 5}``;
        None: every pair).  Pairs that are not candidates (position 0) are left out and counted.  Per user with m >= 1
        relevant candidate pairs at positions p_t among C candidates: hits(k) = #{p_t <= k}, precision@k = hits / k,
        recall@k = hits / m, hit_rate@k = [hits > 0], ndcg@k (binary gains), mrr = 1 / min p_t and
        auc = sum_t (C - m - (p_t - 1 - a_t)) / (m (C - m)) with a_t the relevant pairs before t (not defined for
        C == m).  Each metric is the mean over those users (NaN without any).  ``k``: an int or a list of ints >= 1.

        Returns a dict: ``users`` (evaluated), ``skipped_users`` (users with rows but no relevant candidate pair),
        ``pairs`` (distinct pairs), ``not_candidates`` (pairs at position 0), ``mrr``, ``auc`` and ``precision@k``,
        ``recall@k``, ``ndcg@k``, ``hit_rate@k`` for each k."""
        self._check_whole_model()
        ks, rel_ids = self._ranking_args(k, relevant)
        rows, position, candidates = self._heldout(data, exclude_seen, weights)
        return ranking_metrics(rows[:, 0], rows[:, 1], rows[:, 2], position, candidates, ks, rel_ids)

    # ------------------------------------------------------------------ fold-in of new users (not in the reference)
    def _encode_new(self, data, side):
        """(rows (N, 3) int32 in the training column order, labels of the new entities in order of first appearance).
        Column ``side`` (0: users, 1: items) of ``data`` holds new entities, numbered by first appearance (the training
        theta / eta is never consulted); the other two columns are encoded against the training dictionaries, and rows
        with an unseen entry are dropped with ``Encoder.transform``'s warning.  An entity whose rows are all dropped
        keeps its place (uniform start, no iterations)."""
        import pandas as pd
        from .encode import _columns
        cols, _ = _columns(data)
        own = np.asarray(cols[side])
        fixed = 1 - side
        names = ("users", "items")
        enc = self.data_handler
        if enc:  # labels as the encoder makes them: str(value)
            if own.dtype.kind in "iu":
                codes, uniq = pd.factorize(own)
            else:
                if any(v is None or (isinstance(v, float) and v != v) for v in own.tolist()):
                    raise AssertionError("Data contains missing values. Aborting.")
                codes, uniq = pd.factorize(np.array([str(v) for v in own.tolist()], dtype=object))
            labels = np.array([str(v) for v in np.asarray(uniq).tolist()], dtype=object)
            rows, keep = (enc.transform_items if side == 0 else enc.transform_users)(data, self.logger)
        else:
            if len(own) and (not np.issubdtype(own.dtype, np.integer) or own.min() < 0):
                raise ValueError(f"after fit_encoded the {names[side][:-1]} column holds non-negative integer ids")
            codes, uniq = pd.factorize(own.astype(np.int64))
            labels = np.asarray(uniq, dtype=np.int64)
            other, rating = np.asarray(cols[fixed]), np.asarray(cols[2])
            for name, col in ((names[fixed], other), ("ratings", rating)):
                if len(col) and not np.issubdtype(col.dtype, np.integer):
                    raise ValueError(f"after fit_encoded the {name} column holds encoded integer ids")
            keep = np.ones(len(own), dtype=bool)
            tops = (self.m + 1, self.p + 1)
            for name, col, top in ((names[fixed], other, tops[side]), ("ratings", rating, len(self.ratings))):
                bad = keep & ((col < 0) | (col >= top))
                unseen = np.unique(col[bad])
                if len(unseen):
                    self.logger.warning(f"The {name} {', '.join(str(v) for v in unseen.tolist())} are in the test set "
                                        f"but weren't in the train set so I'll remove them.")
                keep &= ~bad
            rows = np.stack([other[keep], rating[keep]], 1).astype(np.int32)
        out = np.empty((int(keep.sum()), 3), dtype=np.int32)
        out[:, side] = np.asarray(codes)[keep]
        out[:, fixed] = rows[:, 0]
        out[:, 2] = rows[:, 1]
        return out, labels

    def _fold_runs(self, rows, n_new, iterations, tol, each=None, items=False):
        """(thetas, iterations): theta (n_new, K) -- eta (n_new, L) with ``items`` -- and the iterations used of every
        restart, in ``self.results`` order; ``each(ctx)`` runs after each restart's fold-in while its parameters are
        selected (recommend_new adds the slot there)."""
        ctx, restarts = self._restarts()
        thetas, iters = [], []
        for _ in restarts:
            t, it = (ctx.fold_in_items if items else ctx.fold_in)(rows, n_new, iterations, tol)
            thetas.append(t)
            iters.append(it)
            if each is not None:
                each(ctx)
        return thetas, iters

    @staticmethod
    def _fold_args(iterations, tol):
        if isinstance(iterations, (bool, np.bool_)) or not isinstance(iterations, (int, np.integer)) or iterations < 0:
            raise ValueError(f"iterations must be a non-negative integer, got {iterations!r}")
        if tol is not None and not (isinstance(tol, (int, float, np.integer, np.floating)) and np.isfinite(tol)):
            raise ValueError(f"tol must be None or a finite number, got {tol!r}")
        return int(iterations), (None if tol is None else float(tol))

    def fold_in(self, data, iterations=100, tol=None):
        """theta of users that were not in the training data, from their ratings: ``iterations`` steps of the theta
        half of the M-step with every restart's eta and p held fixed, from a uniform start (``tol``: a user stops once
        no entry of its theta moves by more than ``tol``).  ``data``: users, items, ratings like ``fit``'s (after
        ``fit_encoded``: integer triples, users as any non-negative ids, items and ratings encoded).

        Returns a list of DataFrames, one per restart in ``self.results`` order, each (new users x K) indexed by the
        user labels in order of first appearance in ``data``.  ``self.fold_in_iterations``: a DataFrame (new users x
        restarts) of the iterations each user ran.  The model itself is left as it is."""
        import pandas as pd
        self._check_whole_model()
        iterations, tol = self._fold_args(iterations, tol)
        rows, labels = self._encode_new(data, 0)
        thetas, iters = self._fold_runs(rows, len(labels), iterations, tol)
        index = pd.Index(labels, name="users") if len(labels) else pd.Index([], name="users")
        self.fold_in_iterations = pd.DataFrame(np.stack(iters, 1) if iters else np.zeros((len(labels), 0)),
                                               index=index)
        return [pd.DataFrame(t, index=index) for t in thetas]

    def recommend_new(self, data, n=10, exclude_seen=True, weights=None, iterations=100, tol=None, candidates=None):
        """``recommend`` for users that were not in the training data: each restart scores with the theta its own
        ``fold_in`` gives them (same arguments as ``fold_in``), the scores are averaged over the restarts.  Returns
        the frame ``recommend`` returns (users, items, score, rank), users in order of first appearance in ``data``;
        ``exclude_seen`` leaves out the items a user has in ``data``; ``candidates`` as in ``recommend``: only these
        items are scored and ranked."""
        import pandas as pd
        self._check_whole_model()
        n, w = self._recommend_args(n, weights)
        cand = None if candidates is None else self._candidate_ids(candidates)
        iterations, tol = self._fold_args(iterations, tol)
        rows, labels = self._encode_new(data, 0)
        enc = self.data_handler
        item_labels = np.asarray(enc.item_labels(), dtype=object) if enc else None
        n_new = len(labels)
        ctx = self._ctx(self._device_list()[0])
        with self._recommend_session(ctx, w, False):
            thetas, iters = self._fold_runs(rows, n_new, iterations, tol, each=lambda c: c.recommend_add())
            self.fold_in_iterations = pd.DataFrame(np.stack(iters, 1), index=pd.Index(labels, name="users"))
            theta = np.stack(thetas)                                  # (restarts, new users, K)
            if exclude_seen:
                order = np.lexsort((rows[:, 1], rows[:, 0]))
                counts = np.bincount(rows[:, 0], minlength=n_new)
                seen_off = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
                seen_items = rows[order, 1]

            def query(b, e):
                seen = (seen_off[b:e + 1] - seen_off[b], seen_items[seen_off[b]:seen_off[e]]) if exclude_seen else None
                if cand is None:
                    return ctx.recommend_query_theta(theta[:, b:e], n, seen)
                return ctx.recommend_query_theta(theta[:, b:e], n, seen, candidates=cand)
            return self._top_n_frame(query, n, labels, item_labels)

    def fold_in_items(self, data, iterations=100, tol=None):
        """eta of items that were not in the training data, from their ratings: ``iterations`` steps of the eta half of
        the M-step with every restart's theta and p held fixed, from a uniform start (``tol`` as in ``fold_in``).
        ``data``: users, items, ratings like ``fit``'s; every item of it is new (the training eta is never consulted),
        users and ratings are encoded against the training dictionaries and rows with an unseen user or rating are
        dropped with ``predict``'s warning (after ``fit_encoded``: integer triples, items as any non-negative ids, users
        and ratings encoded).

        Returns a list of DataFrames, one per restart in ``self.results`` order, each (new items x L) indexed by the
        item labels in order of first appearance in ``data``.  ``self.fold_in_items_iterations``: a DataFrame (new
        items x restarts) of the iterations each item ran.  The model itself is left as it is."""
        import pandas as pd
        self._check_whole_model()
        iterations, tol = self._fold_args(iterations, tol)
        rows, labels = self._encode_new(data, 1)
        etas, iters = self._fold_runs(rows, len(labels), iterations, tol, items=True)
        index = pd.Index(labels, name="items") if len(labels) else pd.Index([], name="items")
        self.fold_in_items_iterations = pd.DataFrame(np.stack(iters, 1) if iters else np.zeros((len(labels), 0)),
                                                     index=index)
        return [pd.DataFrame(e, index=index) for e in etas]

    def recommend_with_new_items(self, data, users=None, n=10, exclude_seen=True, weights=None, iterations=100,
                                 tol=None):
        """``recommend`` over the training items plus the new items of ``data``: each restart scores the new items with
        the eta its own ``fold_in_items`` gives them (same arguments), the scores are averaged over the restarts.
        Returns the frame ``recommend`` returns (users, items, score, rank) for training users (``users`` as in
        ``recommend``); ``exclude_seen`` leaves out a user's training items and the new items the user rated in
        ``data``.  An item label of ``data`` that is also a training item is refused (ValueError)."""
        import pandas as pd
        self._check_whole_model()
        n, w = self._recommend_args(n, weights)
        iterations, tol = self._fold_args(iterations, tol)
        rows, labels = self._encode_new(data, 1)
        enc = self.data_handler
        n_items = self.m + 1
        if enc:
            train_items = np.asarray(enc.item_labels(), dtype=object)
            known = set(train_items.tolist())
            clash = [x for x in labels.tolist() if x in known]
            item_labels = np.concatenate([train_items, labels]).astype(object)
        else:
            clash = [x for x in labels.tolist() if x < n_items]
            item_labels = np.concatenate([np.arange(n_items, dtype=np.int64), labels]).astype(np.int64)
        if clash:
            raise ValueError(f"items of data are training items, so the frame would be ambiguous: {clash[:10]}")
        ids, user_labels = self._training_users(users)
        n_new = len(labels)
        ctx = self._ctx(self._device_list()[0])
        with self._recommend_session(ctx, w, exclude_seen):
            etas, iters = self._fold_runs(rows, n_new, iterations, tol, each=lambda c: c.recommend_add(), items=True)
            self.fold_in_items_iterations = pd.DataFrame(np.stack(iters, 1), index=pd.Index(labels, name="items"))
            seen = None
            if exclude_seen:  # the training users that rated each new item
                order = np.argsort(rows[:, 1], kind="stable")
                counts = np.bincount(rows[:, 1], minlength=n_new)
                seen = (np.concatenate([[0], np.cumsum(counts)]).astype(np.int64), rows[order, 0])
            ctx.recommend_add_items(np.stack(etas), seen)
            return self._top_n_frame(lambda b, e: ctx.recommend_query(ids[b:e], n), n, user_labels, item_labels)

    def recommend_users_new_items(self, data, n=10, exclude_seen=True, weights=None, iterations=100, tol=None):
        """``recommend_users`` for items that were not in the training data -- the cold-start audience of new items:
        each restart scores with the eta its own ``fold_in_items`` gives them (same arguments), the scores are averaged
        over the restarts.  Returns the frame ``recommend_users`` returns (items, users, score, rank), items in order
        of first appearance in ``data``; ``exclude_seen`` leaves out the users that rated the item in ``data``.  An
        item label of ``data`` that is also a training item is refused (ValueError)."""
        import pandas as pd
        self._check_whole_model()
        n, w = self._recommend_args(n, weights)
        iterations, tol = self._fold_args(iterations, tol)
        rows, labels = self._encode_new(data, 1)
        enc = self.data_handler
        n_items = self.m + 1
        if enc:
            known = set(enc.item_labels())
            clash = [x for x in labels.tolist() if x in known]
            user_labels = np.asarray(enc.user_labels(), dtype=object)
        else:
            clash = [x for x in labels.tolist() if x < n_items]
            user_labels = None
        if clash:
            raise ValueError(f"items of data are training items, so the frame would be ambiguous: {clash[:10]}")
        n_new = len(labels)
        ids = np.arange(n_items, n_items + n_new, dtype=np.int32)
        ctx = self._ctx(self._device_list()[0])
        with self._recommend_session(ctx, w, exclude_seen):
            etas, iters = self._fold_runs(rows, n_new, iterations, tol, each=lambda c: c.recommend_add(), items=True)
            self.fold_in_items_iterations = pd.DataFrame(np.stack(iters, 1), index=pd.Index(labels, name="items"))
            seen = None
            if exclude_seen:  # the training users that rated each new item
                order = np.argsort(rows[:, 1], kind="stable")
                counts = np.bincount(rows[:, 1], minlength=n_new)
                seen = (np.concatenate([[0], np.cumsum(counts)]).astype(np.int64), rows[order, 0])
            ctx.recommend_add_items(np.stack(etas), seen)
            return self._top_n_frame(lambda b, e: ctx.recommend_query_items(ids[b:e], n), n, labels, user_labels,
                                     columns=("items", "users", "score"))

    def _keep_best_run(self, best, res=None):
        """theta / eta / pr / likelihood of restart ``best`` become the model's stored objects
        (src/mmsbm.py:303-311); ``res``: its result dict when it is not in self.results."""
        import pandas as pd
        enc = self.data_handler  # (None after fit_encoded: rows and ratings keep their integer ids)
        res = self.results[best] if res is None else res
        self.theta = pd.DataFrame(res["theta"], index=enc.user_labels() if enc else None)
        self.eta = pd.DataFrame(res["eta"], index=enc.item_labels() if enc else None)
        labels = enc.rating_labels() if enc else range(res["pr"].shape[2])
        self.pr = {lab: pd.DataFrame(res["pr"][:, :, j]) for j, lab in enumerate(labels)}
        self.likelihood = np.float64(res["likelihood"])

    def choose_best_run(self, rats):
        """Index of the first prediction matrix with the highest accuracy (src/mmsbm.py:474-478)."""
        return int(np.argmax([self._compute_stats(a)["accuracy"] for a in rats]))

    # ------------------------------------------------------------------ scoring (src/mmsbm.py:319-369,488-539)
    def score(self, silent=False):
        self._check_has_predictions()
        if self._scored is not None and self._scored[0] is self.prediction_matrix:
            stats = HipEM.final_stats(self._scored[1])  # reduced on the device by predict()
        else:  # a matrix the caller supplied
            stats = self._compute_stats(self.prediction_matrix)
        stats["likelihood"] = self.likelihood
        if not silent:
            self.logger.info(
                f"The final accuracy is {stats['accuracy']}, the one off accuracy is "
                f"{stats['one_off_accuracy']} and the MAE is {stats['mae']}.")
        return {"stats": stats, "objects": {"theta": self.theta, "eta": self.eta, "pr": self.pr}}

    def _compute_stats(self, rat):
        """Scores of a prediction matrix the CALLER supplies (the model's own predictions are scored on
        the device, predict_score_kernel): the same six sums the device returns -- rows with any mass,
        exact hits, hits within one class, |error|, hits and |error| of the weighted prediction
        (src/mmsbm.py:488-528) -- turned into the five scores by HipEM.final_stats."""
        rat = np.asarray(rat, dtype=np.float64)
        truth = np.asarray(self.test[:, 2])
        keep = rat.sum(axis=1) != 0                       # rows without a prediction do not count
        err = np.abs(np.argmax(rat, axis=1) - truth)[keep]
        weighted = (rat @ self.ratings)[keep]
        real = truth[keep]
        raw = (int(keep.sum()), int((err == 0).sum()), int((err <= 1).sum()), int(err.sum()),
               int((np.round(weighted) == real).sum()), float(np.abs(weighted - real).sum()))
        return HipEM.final_stats(raw)

    def compute_likelihood(self, data, theta, eta, pr):
        """src/mmsbm.py:541-553: the likelihood of ``data`` (encoded triples -- the training set
        or any other, e.g. a held-out split) under explicit parameters, evaluated on the device.
        The training set re-uses the resident context; other data gets a context of its own for
        the call."""
        theta, eta, pr = (np.asarray(a, dtype=np.float64) for a in (theta, eta, pr))
        dev = self._device_list()[0]
        train = getattr(self, "train", None)
        if train is not None and (data is train or data_key(data) == self._train_key()):
            ctx = self._ctx(dev)
            self._resident.pop((dev, 0), None)  # slot 0 is overwritten
            ctx.select(0).set_params(theta, eta, pr)
            return ctx.likelihood()
        ctx = HipEM(data, theta.shape[1], eta.shape[1], n_users=theta.shape[0], n_items=eta.shape[0],
                    n_ratings=pr.shape[2], device=dev)
        try:
            ctx.set_params(theta, eta, pr)
            return ctx.likelihood()
        finally:
            ctx.close()

    def _train_key(self):
        if getattr(self, "_train_key_cache", None) is None or self._train_key_cache[0] is not self.train:
            self._train_key_cache = (self.train, data_key(self.train))
        return self._train_key_cache[1]

    # ------------------------------------------------------------------ cross-validation (src/mmsbm.py:371-472)
    def cv_fit(self, data, folds=5):
        """src/mmsbm.py:371-472.  The fold splits are drawn first, in the reference's order (the
        model's RNG is used for nothing else), so the folds are independent jobs: with several
        entries in ``devices`` they run concurrently, one fold per entry at a time (an entry may
        repeat a GPU), each fold's restarts batched on its GPU."""
        n_items = len(set(data.iloc[:, 1]))
        assert folds <= n_items, (
            f"Fold number can't be higher than {n_items} since this is the number of different "
            f"items you have.")
        per_fold = int(n_items / folds)
        temp = data
        splits = []
        for f in range(folds):
            picked = []
            for _, grp in temp.groupby(temp.columns[0]):
                for cnt in range(per_fold, 0, -1):  # as many as the user has, at most per_fold
                    if cnt <= len(grp.index):
                        picked.extend(self.rng.choice(grp.index, cnt, replace=False).tolist())
                        break
            picked = [a for a in picked if str(a) != "0"]
            test = temp.loc[picked, :]
            splits.append((data[~data.index.isin(test.index)], test))
            temp = temp[~temp.index.isin(picked)]

        def run_fold(model, f):
            self.logger.info(f"Running fold {f + 1} of {folds}...")
            train, test = splits[f]
            model.fit(train, silent=True)
            model.prediction_matrix = model.predict(test)
            results = model.score(silent=True)
            return {"stats": results["stats"],
                    "objects": {"theta": model.theta, "eta": model.eta, "pr": model.pr,
                                "rat": model.prediction_matrix}}

        lanes = [int(d) for d in self.devices] if self.devices is not None else [0]
        if len(lanes) == 1 or folds == 1:
            all_results = [run_fold(self, f) for f in range(folds)]
        else:
            def lane(j):  # folds j, j + lanes, ... on GPU lanes[j], through a private model
                child = self._fold_model(lanes[j])
                try:
                    return [(f, run_fold(child, f)) for f in range(j, folds, len(lanes))]
                finally:
                    child._release()
            with ThreadPoolExecutor(max_workers=len(lanes)) as pool:
                parts = list(pool.map(lane, range(min(len(lanes), folds))))
            by_f = dict(x for part in parts for x in part)
            all_results = [by_f[f] for f in range(folds)]
        accuracies = [a["stats"]["accuracy"] for a in all_results]
        kept = all_results[int(np.argmax(accuracies))]["objects"]   # the first best fold (src/mmsbm.py:460-465)
        self.theta, self.eta, self.pr, self.prediction_matrix = (kept[k] for k in ("theta", "eta", "pr", "rat"))
        self.cv_results = all_results
        self.logger.info(f"Ran {folds} folds with accuracies {accuracies}.")
        return accuracies

    def _fold_model(self, device):
        """A model with this one's settings and restart seeds, bound to one GPU."""
        child = MMSBM(self.user_groups, self.item_groups, iterations=self.iterations,
                      sampling=self.sampling, debug=self.debug, backend=self.backend,
                      devices=[device], restarts_per_launch=self.restarts_per_launch,
                      contexts_per_device=self.contexts_per_device, tol=self.tol,
                      check_every=self.check_every)
        child.child_states = self.child_states  # every fold restarts from the same seeds (src/mmsbm.py:441)
        child.logger = self.logger
        return child


def ranking_metrics(users, items, ratings, position, candidates, ks, relevant=None):
    """The dict of ``MMSBM.ranking_score`` from per-row encoded ids, positions and candidate counts (work in
    proportion to the rows).  ``relevant``: a set of rating ids, or None (every pair relevant)."""
    users, items, ratings = (np.asarray(a, dtype=np.int64) for a in (users, items, ratings))
    position, candidates = np.asarray(position, dtype=np.int64), np.asarray(candidates, dtype=np.int64)
    rel_row = np.ones(len(users), dtype=bool) if relevant is None else np.isin(ratings, sorted(relevant))
    # distinct (user, item) pairs: relevant when any of their rows is (the position is the same for every row)
    order = np.lexsort((items, users))
    u, i = users[order], items[order]
    start = np.ones(len(u), dtype=bool)
    start[1:] = (u[1:] != u[:-1]) | (i[1:] != i[:-1])
    pair = np.cumsum(start) - 1
    n_pairs = int(start.sum())
    pu, pp, pc = u[start], position[order][start], candidates[order][start]
    prel = np.zeros(n_pairs, dtype=bool)
    np.logical_or.at(prel, pair, rel_row[order])
    out = {"users": 0, "skipped_users": 0, "pairs": n_pairs, "not_candidates": int((pp == 0).sum())}
    # per user: its relevant candidate pairs sorted by position
    keep = prel & (pp > 0)
    tu, tp, tc = pu[keep], pp[keep], pc[keep]
    o = np.lexsort((tp, tu))
    tu, tp, tc = tu[o], tp[o], tc[o]
    all_users = np.unique(pu)
    ev, first, m = np.unique(tu, return_index=True, return_counts=True)
    n_ev = len(ev)
    out["users"], out["skipped_users"] = n_ev, int(len(all_users) - n_ev)
    grp = np.repeat(np.arange(n_ev), m)
    a = np.arange(len(tu)) - np.repeat(first, m)                   # relevant pairs before each one
    C = tc[first]
    nan = float("nan")
    mean = (lambda v: float(np.mean(v))) if n_ev else (lambda v: nan)
    out["mrr"] = mean(1.0 / tp[first])
    neg = C - m
    ok = neg > 0
    above = np.bincount(grp, weights=(np.repeat(neg, m) - (tp - 1 - a)).astype(np.float64), minlength=n_ev)
    out["auc"] = float(np.mean(above[ok] / (m[ok] * neg[ok]).astype(np.float64))) if ok.any() else nan
    gain = 1.0 / np.log2(tp + 1.0)
    for k in ks:
        inside = tp <= k
        hits = np.bincount(grp, weights=inside.astype(np.float64), minlength=n_ev)
        dcg = np.bincount(grp, weights=np.where(inside, gain, 0.0), minlength=n_ev)
        ideal = np.cumsum(1.0 / np.log2(np.arange(1, max(int(m.max()) if n_ev else 0, 1) + 1) + 1.0))
        idcg = ideal[np.minimum(m, k) - 1] if n_ev else np.zeros(0)
        out[f"precision@{k}"] = mean(hits / k)
        out[f"recall@{k}"] = mean(hits / m)
        out[f"ndcg@{k}"] = mean(dcg / idcg)
        out[f"hit_rate@{k}"] = mean((hits > 0).astype(np.float64))
    return out
