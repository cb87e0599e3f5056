"""sklearn-style estimators over nmf() -- same classes, constructor arguments and methods as the
reference's src/rri_nmf/sklearn_interface.py (NMF_RS_Estimator :14-182, NMF_TM_Estimator :185-345),
so `fit / fit_transform / one_iter / transform / predict / score` keep working while the solver
underneath runs on the MI355X.
"""
import numpy as np
import scipy.sparse as sp
import sklearn.base
from sklearn.model_selection import train_test_split
from sklearn.utils.validation import check_X_y, check_array

from . import nmf as _nmf_module
from .engine import RRIEngine, DeviceCorpus

_RECOMMEND_CHUNK = 1 << 20      # users per rri_topn_rows call of NMF_RS_Estimator.recommend


def _nmf(*a, **kw):
    return _nmf_module.nmf(*a, **kw)


class _FactorPair(object):
    """W / T storage shared by both estimators (sparsify / densify: :42-57, :230-245)."""

    def sparsify(self):
        self.W = self.W.tocsr() if sp.issparse(self.W) else sp.csr_matrix(self.W)
        self.T = self.T.tocsr() if sp.issparse(self.T) else sp.csr_matrix(self.T)

    def densify(self):
        if sp.issparse(self.W):
            self.W = self.W.toarray()
        if sp.issparse(self.T):
            self.T = self.T.toarray()

    def _warm_start(self):
        """the estimator's own factors continue a fit (:105-112, :254-261)"""
        return (self.W if self.W.size > 0 else []), (self.T if self.T.size > 0 else [])

    def _keep(self, soln):
        self.W = soln.pop('W')
        self.T = soln.pop('T')
        self.nmf_outputs = soln


def _observed_mask(X):
    """W_mat of the recommender flavour: 1 where X holds a non-zero rating (sklearn_interface.py:99-102)"""
    if sp.issparse(X):
        M = X.copy()
        M.data = np.ones(M.nnz)
        return M
    M = np.zeros(X.shape)
    M[X.nonzero()] = 1
    return M


def _pairs_pattern(ij, shape):
    """the CSR pattern (ones, sorted columns, no duplicates) of a list of (i, j) pairs, whatever their values"""
    ij = np.asarray(ij, dtype=np.intp)
    A = sp.coo_matrix((np.ones(len(ij)), (ij[:, 0], ij[:, 1])), shape=shape).tocsr()
    A.sum_duplicates()
    A.sort_indices()
    A.data[:] = 1.0
    return A


def _ratings_matrix(values, ij, shape):
    """the ratings as a CSR matrix: what the reference densifies with .toarray() (sklearn_interface.py:78-97)
    stays sparse here -- nmf() then keeps X, W_mat and the residual on the observed entries only"""
    A = sp.coo_matrix((np.asarray(values, dtype=np.float64), (ij[:, 0], ij[:, 1])), shape=shape).tocsr()
    A.sum_duplicates()
    A.eliminate_zeros()      # a zero is "not observed" (W_mat = [X != 0])
    return A


class NMF_RS_Estimator(_FactorPair, sklearn.base.BaseEstimator):
    """Recommender flavour: elementwise-weighted RRI (WRRI) on the observed entries, T entries
    clipped to [0, 1], optional early stopping on a 5 % hold-out (sklearn_interface.py:14-182)."""

    def __init__(self, n, d, k, wr1=0, tr1=0, random_state=0,
                 W=np.array([]), T=np.array([]), max_iter=30, nmf_kwargs={},
                 use_validation_early_stopping=True):
        self.n, self.d, self.k = n, d, k
        self.max_iter = max_iter
        self.wr1, self.tr1 = wr1, tr1
        self.random_state = random_state
        self.min_rating = None
        self.max_rating = None
        self.Xpred = np.array([])
        self.use_validation_early_stopping = use_validation_early_stopping
        self.W, self.T = W, T
        self.nmf_kwargs = nmf_kwargs

    def fit(self, X, y=None):
        """X: (m, 2) index pairs (i, j); y: the m observed values X[i, j]."""
        X, y = check_X_y(X, y)
        self.min_rating, self.max_rating = np.min(y), np.max(y)
        self.seen_ = _pairs_pattern(X, (self.n, self.d))     # every pair given, the hold-out below included (recommend)
        grp = self.nmf_kwargs.get('group')
        if grp is not None:
            # row-sharded fit (one rank's rows, LOCAL row indices in X): the clip bounds of predictions and of the early-stop
            # score are those of ALL ratings, so that every rank scores and stops alike
            mm = grp.gather([self.min_rating, self.max_rating], device=self.nmf_kwargs.get('device', 0))
            self.min_rating, self.max_rating = mm[:, 0].min(), mm[:, 1].max()
        shape = (self.n, self.d)
        if self.use_validation_early_stopping:
            ij_tr, ij_val, r_tr, r_val = train_test_split(X, y, test_size=0.05, random_state=0,
                                                          stratify=None)
            Xtr = _ratings_matrix(r_tr, ij_tr, shape)
            Xv = _ratings_matrix(r_val, ij_val, shape).tocoo()
            vi, vj, vr = Xv.row, Xv.col, Xv.data
            lo, hi = self.min_rating, self.max_rating

            def RMSE_val(X_ignored, W, T):
                pred = np.clip(np.einsum('ij,ji->i', W[vi, :], T[:, vj]), lo, hi)
                return np.sqrt(np.mean((pred - vr) ** 2))

            # same score without bringing W, T to the host: nmf() evaluates callbacks that carry `device_entries`
            # with rri_masked_rmse on the device
            RMSE_val.device_entries = (vi, vj, vr, lo, hi)
            self.early_stop = RMSE_val
        else:
            self.early_stop = False
            Xtr = _ratings_matrix(y, X, shape)
        W_in, T_in = self._warm_start()
        soln = _nmf(Xtr, self.k, max_iter=self.max_iter, max_time=7200, compute_obj_each_iter=True,
                    reset_topic_method=None, early_stop=self.early_stop, project_T_each_iter=False,
                    t_row_sum=1.0, project_W_each_iter=False, w_row_sum=None,
                    W_mat=_observed_mask(Xtr), W_in=W_in, T_in=T_in, reg_w_l1=self.wr1,
                    reg_t_l1=self.tr1, random_state=self.random_state, **self.nmf_kwargs)
        self._keep(soln)
        return self

    def fit_from_Xtr(self, Xtr):
        """builds the (index pairs, values) lists from a ratings matrix and fits.  A DeviceCorpus is taken through one
        to_scipy() download: the weighted fit from a resident corpus is not built."""
        if isinstance(Xtr, DeviceCorpus):
            Xtr = Xtr.to_scipy()
        Xtr = Xtr.tocsr() if sp.issparse(Xtr) else sp.csr_matrix(Xtr)
        rows, cols = Xtr.nonzero()
        return self.fit(np.column_stack((rows, cols)), Xtr.data)

    def fit_corpus(self, train, held=None, keep_seen=True):
        """The fit of `fit` from ratings that are resident: `train` is a DeviceCorpus (DeviceCorpus.from_pairs(index_pairs,
        ratings), or the observed half of its split_entries), and nothing of its size visits the host -- no train_test_split, no
        CSR matrix built on the host, no upload.  The solver runs nmf(train, k, observed_only=True, ...) with the options of `fit`:
        the weighted flavour on a pattern-only handle whose store is built on the device from the corpus.  `held` is a DeviceCorpus
        of held-out ratings for the early stop (scored between sweeps by rri_corpus_entries_error where it lies); with
        use_validation_early_stopping and no `held`, train.split_entries(held_out=0.05, random_state=0) is made, used and closed
        here (the hold-out is then another 5 % than train_test_split's: the same estimator, another draw).  The rating range that
        clips predictions is that of train and held together (DeviceCorpus.value_range).  keep_seen=True downloads the pattern of
        train and held once, after the fit, into seen_ (indptr and indices only) for recommend / rank; keep_seen=False leaves seen_
        None, and recommend(exclude_seen=True) raises.  The default start runs through the handle's products whatever the size
        (fit takes scikit-learn's SVD below 2e7 entries unless nmf_kwargs has device_init=True)."""
        from .corpus_fit import pattern_of
        if not isinstance(train, DeviceCorpus) or (held is not None and not isinstance(held, DeviceCorpus)):
            raise TypeError('fit_corpus takes DeviceCorpus objects: for matrices and pairs there are fit_from_Xtr and fit')
        if tuple(train.shape) != (self.n, self.d) or (held is not None and tuple(held.shape) != (self.n, self.d)):
            raise ValueError('the corpora must be %d x %d' % (self.n, self.d))
        ranges = [c.value_range() for c in (train, held) if c is not None and c.nnz > 0]
        if not ranges:
            raise ValueError('there are no ratings to fit')
        self.min_rating, self.max_rating = min(r[0] for r in ranges), max(r[1] for r in ranges)
        own = ()
        fit_on, stop_on = train, held
        try:
            if self.use_validation_early_stopping and held is None:
                own = train.split_entries(held_out=0.05, random_state=0)
                fit_on, stop_on = own
            if self.use_validation_early_stopping:
                def RMSE_val(X_ignored, W, T):
                    raise NotImplementedError('this early stop is scored on the device (device_corpus)')

                RMSE_val.device_corpus = (stop_on, self.min_rating, self.max_rating)
                self.early_stop = RMSE_val
            else:
                self.early_stop = False
            W_in, T_in = self._warm_start()
            soln = _nmf(fit_on, self.k, max_iter=self.max_iter, max_time=7200, compute_obj_each_iter=True,
                        reset_topic_method=None, early_stop=self.early_stop, project_T_each_iter=False,
                        t_row_sum=1.0, project_W_each_iter=False, w_row_sum=None,
                        observed_only=True, W_in=W_in, T_in=T_in, reg_w_l1=self.wr1,
                        reg_t_l1=self.tr1, random_state=self.random_state, **self.nmf_kwargs)
        finally:
            for c in own:
                c.close()
        self._keep(soln)     # (nmf_outputs['obj_calculator'] re-evaluates on the corpus it was given, while that one is open)
        self.seen_ = None
        if keep_seen:
            seen = pattern_of(train)
            if held is not None and held.nnz > 0:
                seen = (seen + pattern_of(held)).tocsr()
                seen.sum_duplicates()
                seen.sort_indices()
                seen.data[:] = 1.0
            self.seen_ = seen
        return self

    def score_corpus(self, corpus, W=None):
        """RMSE of the clipped reconstruction on the stored entries of a DeviceCorpus, scored on the device where the corpus lies
        (rri_corpus_entries_error on a factors-only handle): what score(corpus.to_scipy()) returns, to rounding, without the
        download.  W: the rows of folded users (transform_corpus), m x k, scored with the fitted T against a corpus of m x d; None:
        the fitted W."""
        from .corpus_fit import entries_error
        if np.ndim(self.T) != 2 or (W is None and np.ndim(self.W) != 2):
            raise ValueError('the estimator is not fitted: it has no W and T')
        T = self.T.toarray() if sp.issparse(self.T) else np.asarray(self.T)
        if W is None:
            W = self.W.toarray() if sp.issparse(self.W) else np.asarray(self.W)
        else:
            W = self._folded_rows(W, T, (('corpus', corpus),))
        eng = RRIEngine(W.shape[0], T.shape[1], W.shape[1], dtype=np.float64, weighted=False, device=self.nmf_kwargs.get('device', 0))
        try:        # factors only: such a handle holds nothing of size n x d
            eng.set_W(W)
            eng.set_T(T)
            return entries_error(eng, corpus, clip=(self.min_rating, self.max_rating))['rmse']
        finally:
            eng.close()

    @staticmethod
    def _folded_rows(W, T, corpora):
        """the W of folded users as a float64 (m, k) array beside the fitted T; the corpora given with it must be m x d"""
        W = np.asarray(W.toarray() if sp.issparse(W) else W, dtype=np.float64)
        if W.ndim != 2 or W.shape[1] != T.shape[0]:
            raise ValueError('W must be an (m, %d) array of folded rows, not of shape %s' % (T.shape[0], W.shape))
        for what, c in corpora:
            if isinstance(c, DeviceCorpus) and tuple(c.shape) != (W.shape[0], T.shape[1]):
                raise ValueError('with W of %d rows, %s must be a DeviceCorpus of shape %d x %d' % (W.shape[0], what, W.shape[0], T.shape[1]))
        return W

    def _factors_engine(self, corpora, W=None):
        """a factors-only handle holding the fitted W -- or the (m, k) rows of folded users given as W -- and the fitted T (nothing of
        size n x d), after the corpora have been checked"""
        if np.ndim(self.T) != 2 or (W is None and np.ndim(self.W) != 2):
            raise ValueError('the estimator is not fitted: it has no W and T')
        for what, c in corpora:
            if c is not None and not isinstance(c, DeviceCorpus):
                raise TypeError('%s must be a DeviceCorpus, not %s' % (what, type(c).__name__))
        T = self.T.toarray() if sp.issparse(self.T) else np.asarray(self.T)
        if W is None:
            W = self.W.toarray() if sp.issparse(self.W) else np.asarray(self.W)       # sparsify() was called: dense copies
        else:
            W = self._folded_rows(W, T, corpora)
        eng = RRIEngine(W.shape[0], T.shape[1], W.shape[1], dtype=np.float64, weighted=False, device=self.nmf_kwargs.get('device', 0))
        try:
            eng.set_W(W)
            eng.set_T(T)
        except Exception:
            eng.close()
            raise
        return eng

    def recommend_corpus(self, users=None, n_items=10, exclude=None, W=None):
        """`recommend` against a resident exclusion: the n_items best items for each of `users` (row indices, any order, duplicates
        allowed; None: every user), leaving out for user i the stored entries of row i of `exclude` -- a DeviceCorpus of the
        estimator's shape, typically the corpus split_entries was called on (train and held-out together), or None --, read where
        it lies (rri_corpus_topn_rows): no seen_, no copy of the excluded pairs on the host.  (items int32 (m, n_items), scores
        float64 (m, n_items)), the items and scores `recommend` returns when seen_ is that corpus's pattern.  W: the (m, k) rows of
        folded users (transform_corpus) instead of the fitted W: `users` index those rows and `exclude` is then m x d."""
        from .corpus_rank import topn_rows
        eng = self._factors_engine((('exclude', exclude),), W)
        try:
            n = eng.n
            users = np.arange(n, dtype=np.int64) if users is None else np.asarray(users, dtype=np.int64).reshape(-1)
            if users.size and (users.min() < 0 or users.max() >= n):
                raise ValueError('users must be row indices in [0, %d)' % n)
            n_items = int(n_items)
            items = np.empty((users.size, max(n_items, 0)), dtype=np.int32)
            scores = np.empty((users.size, max(n_items, 0)), dtype=np.float64)
            for lo in range(0, users.size, _RECOMMEND_CHUNK):       # the exclusion is indexed by the user: passed whole to every chunk
                u = users[lo:lo + _RECOMMEND_CHUNK]
                items[lo:lo + u.size], scores[lo:lo + u.size] = topn_rows(eng, u, n_items, exclude=exclude,
                                                                          clip=(self.min_rating, self.max_rating))[:2]
        finally:
            eng.close()
        return items, scores

    def rank_corpus(self, targets, exclude=None, W=None):
        """`rank` for pairs that are resident: the place of every stored entry (user i, item j) of the DeviceCorpus `targets` (the
        estimator's shape) among user i's items, counted on the device where the corpus lies (rri_corpus_rank_entries): (rank int32
        per canonical entry in corpus order, eligible int32 per row; -1 for a user without entries, who is not scored).  `exclude`
        as in recommend_corpus; an entry that is itself excluded, or whose prediction is NaN, gets rank -1.  W as in recommend_corpus:
        the corpora are then m x d."""
        from .corpus_rank import rank_entries
        eng = self._factors_engine((('targets', targets), ('exclude', exclude)), W)
        try:
            if targets is None or tuple(targets.shape) != (eng.n, eng.d):
                raise ValueError('targets must be a DeviceCorpus of shape %d x %d' % (eng.n, eng.d))
            res = rank_entries(eng, targets, exclude=exclude, clip=(self.min_rating, self.max_rating), values=False)
        finally:
            eng.close()
        return res['rank'], res['eligible']

    def ranking_score_corpus(self, targets, n_items=10, exclude=None, relevant_from=None, W=None):
        """`ranking_score` for pairs that are resident: the same dict, formula for formula, over the stored entries of the
        DeviceCorpus `targets` whose value is at least relevant_from (None: all), ranked and summed on the device
        (rri_corpus_ranking_metrics): a dozen doubles come back, not one rank per pair, and neither the corpus nor seen_ is
        downloaded.  `exclude` and W as in recommend_corpus.  The metrics agree with ranking_score's to the order of the sums."""
        from .corpus_rank import ranking_metrics
        n_items = int(n_items)
        if n_items < 1:
            raise ValueError('n_items must be a positive integer, not %d' % n_items)
        eng = self._factors_engine((('targets', targets), ('exclude', exclude)), W)
        try:
            if targets is None or tuple(targets.shape) != (eng.n, eng.d):
                raise ValueError('targets must be a DeviceCorpus of shape %d x %d' % (eng.n, eng.d))
            return ranking_metrics(eng, targets, n_items, exclude=exclude, relevant_from=relevant_from)
        finally:
            eng.close()

    def transform_corpus(self, new):
        """`transform` for ratings that are resident: `new` is a DeviceCorpus of m x d (any m) whose stored entries are the new
        users' ratings, and nothing of its size visits the host.  The solver runs nmf(new, k, observed_only=True, fold_in=True, ...)
        with the options of `transform`: four sweeps with T fixed on a pattern-only handle whose store is built on the device, each
        sweep's W half one launch (include/rri_fold.h; k <= 64, a larger rank runs launch by launch).  Returns W_new (m x k), which
        recommend_corpus, rank_corpus, ranking_score_corpus and score_corpus take as W=."""
        if not isinstance(new, DeviceCorpus):
            raise TypeError('transform_corpus takes a DeviceCorpus, not %s: for matrices there is transform' % type(new).__name__)
        if np.ndim(self.T) != 2:
            raise ValueError('the estimator is not fitted: it has no T')
        if new.shape[1] != self.d:
            raise ValueError('the corpus has %d columns, the estimator %d' % (new.shape[1], self.d))
        T = self.T.toarray() if sp.issparse(self.T) else self.T
        soln = _nmf(new, self.k, max_iter=4, max_time=7200, project_W_each_iter=False,
                    project_T_each_iter=False, observed_only=True, fold_in=True, T_in=T, fix_T=True,
                    reg_w_l1=self.wr1, reg_t_l1=self.tr1, t_row_sum=1.0, w_row_sum=None,
                    reset_topic_method='random', random_state=self.random_state, **self.nmf_kwargs)
        return soln['W']

    def ranking_score_new_users(self, new, n_items=10, n_held=None, held_out=None, min_observed=1, relevant_from=None, random_state=None):
        """The ranking metrics of users the fit never saw (strong generalisation), end to end on the device: `new` is a DeviceCorpus
        of m x d holding their ratings.  Every user gives up part of the ratings (new.split_rows: n_held per user, or the share
        held_out; neither given: held_out=0.2; every user keeps at least min_observed), is folded in from the ratings kept
        (transform_corpus), and the ratings given up are ranked among the items the user has not kept (ranking_score_corpus with
        exclude=observed and W=the folded rows).  It is exactly that composition; random_state=None is the estimator's own.  Returns
        the dict of ranking_score_corpus with two integer keys added: observed_entries and held_entries."""
        if not isinstance(new, DeviceCorpus):
            raise TypeError('ranking_score_new_users takes a DeviceCorpus, not %s' % type(new).__name__)
        if n_held is None and held_out is None:
            held_out = 0.2
        DeviceCorpus._split_rows_request(n_held, held_out, min_observed)
        if int(n_items) < 1:
            raise ValueError('n_items must be a positive integer, not %d' % int(n_items))
        if np.ndim(self.T) != 2:
            raise ValueError('the estimator is not fitted: it has no T')
        if new.shape[1] != self.d:
            raise ValueError('the corpus has %d columns, the estimator %d' % (new.shape[1], self.d))
        observed, held = new.split_rows(n_held=n_held, held_out=held_out, min_observed=min_observed,
                                        random_state=self.random_state if random_state is None else random_state)
        try:
            W_new = self.transform_corpus(observed)
            out = dict(self.ranking_score_corpus(held, n_items, exclude=observed, relevant_from=relevant_from, W=W_new))
            out['observed_entries'], out['held_entries'] = int(observed.nnz), int(held.nnz)
            return out
        finally:
            observed.close()
            held.close()

    def transform(self, Xnew):
        """fold new rows in against the fitted T (transform_corpus: the same from a DeviceCorpus, one launch per sweep)"""
        soln = _nmf(Xnew, self.k, max_iter=4, max_time=7200, project_W_each_iter=False,
                    project_T_each_iter=False, W_mat=_observed_mask(Xnew), T_in=self.T, fix_T=True,
                    reg_w_l1=self.wr1, reg_t_l1=self.tr1, t_row_sum=1.0, w_row_sum=None,
                    reset_topic_method='random', random_state=self.random_state, **self.nmf_kwargs)
        return soln['W']

    def make_Xpred(self):
        """the full clipped reconstruction, n x d dense (sklearn_interface.py:158-161): kept for callers that want it;
        predict / score below evaluate only the entries they are asked for"""
        if self.Xpred.size == 0:
            self.Xpred = np.clip(np.dot(self.W, self.T), a_min=self.min_rating, a_max=self.max_rating)

    def _predict_entries(self, i, j):
        """clip(W T)[i, j] for index arrays i, j without forming the n x d product"""
        if self.Xpred.size > 0:
            return self.Xpred[i, j]
        W = self.W.toarray() if sp.issparse(self.W) else self.W
        T = self.T.toarray() if sp.issparse(self.T) else self.T
        out = np.empty(len(i))
        for lo in range(0, len(i), 1 << 20):          # chunks: the gathered rows are 2^20 x k doubles
            sl = slice(lo, lo + (1 << 20))
            out[sl] = np.einsum('ek,ke->e', W[i[sl], :], T[:, j[sl]])
        return np.clip(out, self.min_rating, self.max_rating)

    def recommend(self, users=None, n_items=10, exclude_seen=True):
        """The n_items best items for each of `users` (row indices, any order, duplicates allowed; None: every user), scored
        and selected on the device (rri_topn_rows): (items int32 (m, n_items), scores float64 (m, n_items)).  Items are ranked by
        the unclipped prediction W[i, :] T[:, j], larger first, equal predictions by the smaller item; the scores returned are
        clipped to the rating range, the numbers `predict` gives for those pairs.  exclude_seen leaves out the pairs given to fit
        (seen_, the hold-out included); a user with fewer than n_items items left gets item -1 and score NaN in the last slots.
        No n x d product is formed anywhere, and there is no host route: without a GPU the call raises RRIHipUnavailable.
        recommend_corpus excludes the entries of a resident corpus instead of seen_, without a copy of them on the host."""
        if np.ndim(self.W) != 2 or np.ndim(self.T) != 2:
            raise ValueError('the estimator is not fitted: it has no W and T')
        if exclude_seen and getattr(self, 'seen_', None) is None:
            raise ValueError('exclude_seen=True needs the pairs given to fit (seen_), which this estimator does not have')
        W = self.W.toarray() if sp.issparse(self.W) else np.asarray(self.W)       # sparsify() was called: dense copies
        T = self.T.toarray() if sp.issparse(self.T) else np.asarray(self.T)
        n, d = W.shape[0], T.shape[1]
        users = np.arange(n, dtype=np.int64) if users is None else np.asarray(users, dtype=np.int64).reshape(-1)
        if users.size and (users.min() < 0 or users.max() >= n):
            raise ValueError('users must be row indices in [0, %d)' % n)
        n_items = int(n_items)
        items = np.empty((users.size, max(n_items, 0)), dtype=np.int32)
        scores = np.empty((users.size, max(n_items, 0)), dtype=np.float64)
        eng = RRIEngine(n, d, W.shape[1], dtype=np.float64, weighted=False, device=self.nmf_kwargs.get('device', 0))
        try:        # factors only: such a handle holds nothing of size n x d
            eng.set_W(W)
            eng.set_T(T)
            for lo in range(0, users.size, _RECOMMEND_CHUNK):
                u = users[lo:lo + _RECOMMEND_CHUNK]
                items[lo:lo + u.size], scores[lo:lo + u.size] = eng.topn_rows(
                    u, n_items, exclude=self.seen_[u] if exclude_seen else None, clip=(self.min_rating, self.max_rating))
        finally:
            eng.close()
        return items, scores

    def _pairs_of(self, X, y=None):
        """(i, j, y) of what rank / ranking_score are given: (m, 2) index pairs as predict takes them, or an n x d matrix (dense
        or scipy sparse) whose stored non-zeros are the pairs, in the order of X.nonzero(), their values standing in for a y
        that is not given.  A dense array with two columns is read as pairs."""
        n, d = np.shape(self.W)[0], np.shape(self.T)[1]
        if sp.issparse(X) or (np.ndim(X) == 2 and np.shape(X) == (n, d) and d != 2):
            if X.shape != (n, d):
                raise ValueError('a matrix of pairs must be %d x %d, not %r' % (n, d, X.shape))
            if sp.issparse(X):
                C = X.tocoo()                   # what X.nonzero() does, keeping the values
                keep = C.data != 0
                i, j, vals = C.row[keep], C.col[keep], C.data[keep]
            else:
                i, j = np.nonzero(X)
                vals = np.asarray(X)[i, j]
            y = vals if y is None else y
        else:
            ij = np.asarray(check_array(X, ensure_min_samples=0), dtype=np.int64) if np.size(X) else np.zeros((0, 2), dtype=np.int64)
            if ij.ndim != 2 or ij.shape[1] != 2:
                raise ValueError('pairs must be an (m, 2) array of (row, column) indices')
            i, j = ij[:, 0], ij[:, 1]
        i, j = np.asarray(i, dtype=np.int64), np.asarray(j, dtype=np.int64)
        if i.size and (i.min() < 0 or i.max() >= n or j.min() < 0 or j.max() >= d):
            raise ValueError('pairs must be (row, column) indices inside %d x %d' % (n, d))
        if y is not None:
            y = np.asarray(y, dtype=np.float64).ravel()
            if y.size != i.size:
                raise ValueError('y must hold one value per pair: %d, not %d' % (i.size, y.size))
        return i, j, y

    def rank(self, X, exclude_seen=True):
        """The place of each given pair (user i, item j) among user i's items, counted on the device (rri_rank_entries):
        (rank int32 (m,), eligible int32 (m,)), aligned with the pairs as given -- a pair given twice gets its answer twice.  X is
        (m, 2) index pairs or an n x d matrix whose stored non-zeros are the pairs (the order is that of X.nonzero()).  rank is
        the number of the user's eligible items that `recommend` would list before item j (by the unclipped prediction, larger
        first, equal predictions by the smaller item; the user's other pairs compete like any item), eligible the number of items
        the user has to choose from.  exclude_seen leaves out the pairs given to fit (seen_, the hold-out included); a pair that
        is itself in seen_ is not eligible and gets rank -1 -- it is not taken out of the exclusion silently --, as does a pair
        whose prediction is NaN.  No n x d product is formed, and there is no host route: without a GPU the call raises
        RRIHipUnavailable.  A DeviceCorpus is taken as its matrix through one to_scipy() download: into this method a route that
        reads a resident corpus is not built, because its answer is aligned with pairs on the host; rank_corpus ranks the corpus
        where it lies."""
        if isinstance(X, DeviceCorpus):
            X = X.to_scipy()
        if np.ndim(self.W) != 2 or np.ndim(self.T) != 2:
            raise ValueError('the estimator is not fitted: it has no W and T')
        if exclude_seen and getattr(self, 'seen_', None) is None:
            raise ValueError('exclude_seen=True needs the pairs given to fit (seen_), which this estimator does not have')
        i, j, _ = self._pairs_of(X)
        W = self.W.toarray() if sp.issparse(self.W) else np.asarray(self.W)       # sparsify() was called: dense copies
        T = self.T.toarray() if sp.issparse(self.T) else np.asarray(self.T)
        n, d = W.shape[0], T.shape[1]
        targets = _pairs_pattern(np.column_stack((i, j)), (n, d))                 # every pair once, columns ascending
        users = np.flatnonzero(np.diff(targets.indptr))
        rank_csr = np.empty(targets.nnz, dtype=np.int32)
        eligible_user = np.full(n, -1, dtype=np.int32)
        eng = RRIEngine(n, d, W.shape[1], dtype=np.float64, weighted=False, device=self.nmf_kwargs.get('device', 0))
        try:        # factors only: such a handle holds nothing of size n x d
            eng.set_W(W)
            eng.set_T(T)
            for lo in range(0, users.size, _RECOMMEND_CHUNK):
                u = users[lo:lo + _RECOMMEND_CHUNK]
                res = eng.rank_entries(u, targets[u], exclude=self.seen_[u] if exclude_seen else None,
                                       clip=(self.min_rating, self.max_rating))
                # the users ascend and each has all its pairs in one chunk: the chunk's targets are one stretch of the CSR
                rank_csr[targets.indptr[u[0]]:targets.indptr[u[-1] + 1]] = res.rank
                eligible_user[u] = res.eligible
        finally:
            eng.close()
        keys = np.repeat(np.arange(n, dtype=np.int64), np.diff(targets.indptr)) * d + targets.indices
        pos = np.searchsorted(keys, i * d + j)
        return rank_csr[pos], eligible_user[i]

    def ranking_score(self, X, y=None, n_items=10, exclude_seen=True, relevant_from=None):
        """Ranking metrics of held-out pairs from their full-row ranks (`rank`): a dict.  X as in `rank`; with relevant_from
        only the pairs whose value (y, or the stored value of a matrix X) is at least relevant_from are targets; a pair given
        twice is one target.  n_items (N) is any positive integer.  With P_u the number of eligible targets of user u, L_u the
        user's eligible count and r_0 < ... < r_{P-1} the user's target ranks:
          hit_rate   mean over users with P_u >= 1 of [any r < N]
          precision  ... of #{r < N} / N
          recall     ... of #{r < N} / P_u
          ndcg       ... of sum_{r < N} 1 / log2(r + 2) over sum_{p < min(N, P_u)} 1 / log2(p + 2)
          mrr        ... of 1 / (1 + r_0)
          auc        mean over users with P_u >= 1 and L_u > P_u of 1 - sum_a (r_a - a) / (P_u (L_u - P_u))
          mean_percentile_rank   mean over eligible targets with L_u > 1 of r / (L_u - 1)
        and n_items, users (how many were averaged), targets, targets_not_eligible (rank -1: in seen_ under exclude_seen, or a
        NaN prediction).  Without an eligible target the metrics are NaN and the counts say why.  Computed on the host in
        float64; each rank of a row-sharded fit scores its own rows.  A DeviceCorpus is taken as its matrix through one
        to_scipy() download: into this method a route that reads a resident corpus is not built; ranking_score_corpus ranks the
        corpus where it lies and sums the metrics on the device."""
        if isinstance(X, DeviceCorpus):
            X = X.to_scipy()
        n_items = int(n_items)
        if n_items < 1:
            raise ValueError('n_items must be a positive integer, not %d' % n_items)
        if np.ndim(self.W) != 2 or np.ndim(self.T) != 2:
            raise ValueError('the estimator is not fitted: it has no W and T')
        i, j, y = self._pairs_of(X, y)
        if relevant_from is not None:
            if y is None:
                raise ValueError('relevant_from needs the values y of the pairs')
            keep = y >= relevant_from
            i, j = i[keep], j[keep]
        d = np.shape(self.T)[1]
        key, first = np.unique(i * d + j, return_index=True)                     # every pair once
        i, j = i[first], j[first]
        rank, eligible = self.rank(np.column_stack((i, j)), exclude_seen=exclude_seen)
        ok = rank >= 0
        out = {'n_items': n_items, 'targets': int(i.size), 'targets_not_eligible': int((~ok).sum())}
        users, uid = np.unique(i[ok], return_inverse=True)
        out['users'] = int(users.size)
        names = ('hit_rate', 'precision', 'recall', 'ndcg', 'mrr', 'auc', 'mean_percentile_rank')
        if users.size == 0:
            out.update((name, float('nan')) for name in names)
            return out
        r, L = rank[ok].astype(np.float64), eligible[ok].astype(np.float64)
        order = np.lexsort((r, uid))                                              # by user, the user's ranks ascending
        r, L, uid = r[order], L[order], uid[order]
        P = np.bincount(uid).astype(np.float64)
        start = np.concatenate(([0], np.cumsum(P)[:-1])).astype(np.int64)
        a = np.arange(r.size) - start[uid]                                        # the target's place among its user's targets
        Lu = L[start]
        hit = r < n_items
        hits = np.bincount(uid, weights=hit)
        ideal = np.concatenate(([0.0], np.cumsum(1.0 / np.log2(np.arange(min(n_items, int(P.max()))) + 2.0))))
        out['hit_rate'] = float(np.mean(hits > 0))
        out['precision'] = float(np.mean(hits / n_items))
        out['recall'] = float(np.mean(hits / P))
        out['ndcg'] = float(np.mean(np.bincount(uid, weights=hit / np.log2(r + 2.0)) / ideal[np.minimum(n_items, P).astype(np.int64)]))
        out['mrr'] = float(np.mean(1.0 / (1.0 + r[start])))
        room = Lu > P
        out['auc'] = float(np.mean(1.0 - np.bincount(uid, weights=r - a)[room] / (P[room] * (Lu[room] - P[room])))) if room.any() else float('nan')
        wide = L > 1
        out['mean_percentile_rank'] = float(np.mean(r[wide] / (L[wide] - 1.0))) if wide.any() else float('nan')
        return out

    def predict(self, X):
        X = check_array(X)
        # the reference indexes with the float array check_array returns, which modern numpy rejects
        idx = np.asarray(X, dtype=np.intp)
        return self._predict_entries(idx[:, 0], idx[:, 1])

    def score(self, X, y=np.array([])):
        """RMSE of the clipped reconstruction on the given entries (sklearn_interface.py:172-182).  A DeviceCorpus is taken as its
        matrix through one to_scipy() download: the weighted fit from a resident corpus is not built."""
        if isinstance(X, DeviceCorpus):
            X = X.to_scipy()
        if y.size > 0:
            if sp.issparse(X):
                X = X.toarray()
            return np.sqrt(np.mean((y - self.predict(X)) ** 2))
        if sp.issparse(X):
            C = X.tocoo()
            keep = C.data != 0
            i, j, v = C.row[keep], C.col[keep], C.data[keep]
        else:
            i, j = X.nonzero()
            v = X[i, j]
        return np.sqrt(np.mean((v - self._predict_entries(i, j)) ** 2))


def _all_nonnegative(X):
    """np.all(X >= 0) (sklearn_interface.py:251) without the boolean copy of X, and for a large dense array on several threads
    (numpy's reductions release the GIL): 0.2 s of a 1.8 s fit at 100000 x 10000 went into the plain form.  NaN fails, as there."""
    if isinstance(X, DeviceCorpus):     # counted on the device when the corpus was made
        return X.negatives == 0
    if sp.issparse(X):          # the stored values (scipy refuses `>= 0` on a sparse matrix)
        return bool(np.all(X.tocsr().data >= 0))
    if not isinstance(X, np.ndarray) or X.ndim != 2 or X.size < (1 << 24):
        return bool(np.all(X >= 0))
    from concurrent.futures import ThreadPoolExecutor
    import os
    nt = max(1, min(16, os.cpu_count() or 1))
    cuts = np.linspace(0, X.shape[0], nt + 1).astype(np.int64)
    with ThreadPoolExecutor(nt) as pool:
        mins = list(pool.map(lambda i: X[cuts[i]:cuts[i + 1]].min() if cuts[i + 1] > cuts[i] else 0.0, range(nt)))
    return bool(np.all(np.asarray(mins) >= 0))          # a NaN minimum compares False


class NMF_TM_Estimator(_FactorPair, sklearn.base.BaseEstimator, sklearn.base.TransformerMixin):
    """Topic-model flavour: rows of T on the simplex after every update, rows of W projected at the
    end (sklearn_interface.py:185-345).

    n, d, k: documents, dictionary size, topics; wr1/wr2/tr1/tr2: l1/l2 penalties on W and T;
    handle_tfidf / handle_normalization: preprocess X inside fit/transform; W, T: optional warm
    start; nmf_kwargs: extra keyword arguments for nmf()."""

    def __init__(self, n, d, k, wr1=0, wr2=0, tr1=0, tr2=0, random_state=0,
                 handle_tfidf=False, handle_normalization=False, max_iter=300,
                 W=np.array([]), T=np.array([]), nmf_kwargs={},
                 do_final_project_W=True, keep_resident=False):
        # keep_resident (not in the reference): fit / one_iter on the SAME array X keep its device handle -- X uploaded and
        # preprocessed -- between the calls (nmf.ResidentProblem; the caller must not modify X in place meanwhile); release()
        # frees it.  A scipy sparse X keeps its handle when its preprocessing runs on the device (_takes_holder)
        self.keep_resident = keep_resident
        self._resident = None
        self.n, self.d, self.k = n, d, k
        self.wr1, self.wr2, self.tr1, self.tr2 = wr1, wr2, tr1, tr2
        self.random_state = random_state
        self.handle_tfidf = handle_tfidf
        self.handle_normalization = handle_normalization
        self.max_iter = max_iter
        self.W, self.T = W, T
        self.nmf_kwargs = nmf_kwargs
        self.do_final_project_W = do_final_project_W

    def _preprocess_kwargs(self, idf=None):
        """handle_tfidf / handle_normalization as nmf()'s `preprocess` option (sklearn_interface.py:243-247, 303-306):
        a dense X is then rewritten on the device after the upload instead of on the host before it"""
        if not (self.handle_tfidf or self.handle_normalization):
            return {}
        tf = False if not self.handle_tfidf else (True if idf is None else idf)
        return {'preprocess': {'tfidf': tf, 'normalize': bool(self.handle_normalization)}}

    def _solve(self, X, max_iter, max_time):
        W_in, T_in = self._warm_start()
        kw = dict(self._preprocess_kwargs(), **self.nmf_kwargs)
        if self.keep_resident and self._takes_holder(X, kw):
            if self._resident is None:
                self._resident = _nmf_module.ResidentProblem()
            kw['resident'] = self._resident
        soln = _nmf(X, self.k, max_iter=max_iter, max_time=max_time, project_W_each_iter=False,
                    w_row_sum=1.0, project_T_each_iter=True, t_row_sum=1.0,
                    do_final_project_W=self.do_final_project_W, W_in=W_in, T_in=T_in,
                    reg_w_l1=self.wr1, reg_w_l2=self.wr2, reg_t_l1=self.tr1, reg_t_l2=self.tr2,
                    random_state=self.random_state, **kw)
        if self.handle_tfidf:
            self.idf = soln['idf']
        self._keep(soln)

    @staticmethod
    def _takes_holder(X, kw):
        """keep_resident on a scipy sparse X: nmf() keeps a handle when the preprocessing asked for runs on the device
        (nmf.preprocess_route); where it runs on the host -- a CSR handle and an empty row to normalise, without
        nmf_kwargs' uniform_rows=True -- there is no holder, as for every sparse X before the CSR handle preprocessed on the device"""
        if not sp.issparse(X):      # (a DeviceCorpus too: whatever is asked for runs on the device)
            return True
        spec = _nmf_module._preprocess_spec(kw.get('preprocess'))
        if spec is None:
            return False
        route, _ = _nmf_module._route_of_call(X, spec, kw.get('sparse_X'), kw.get('dtype'), kw.get('device', 0), kw.get('W_mat'),
                                              kw.get('w_row'), bool(kw.get('diagnostics')) or bool(kw.get('store_gradients')),
                                              kw.get('schedule', 'gram'), kw.get('group'), bool(kw.get('uniform_rows')))
        return route == 'device'

    def release(self):
        """free the device handle kept by keep_resident"""
        if self._resident is not None:
            self._resident.close()

    def fit_transform(self, X, y=None):
        assert _all_nonnegative(X), 'X must be non-negative'
        self._solve(X, self.max_iter, 7200)
        return self.W

    def fit(self, X, y=None):
        self.fit_transform(X, y)
        return self

    def one_iter(self, X):
        """one more sweep from the estimator's current factors"""
        self._solve(X, 1, 240)
        return self

    def partial_fit(self, X, y=None, sweeps=3, decay=1.0):
        """Online fit: one batch of documents joins the model (not in the reference).  The first call initialises from its
        batch and runs `sweeps` sweeps -- what fit() does with max_iter = sweeps: one partial_fit on all rows from the same
        start leaves the same W and T bit for bit.  Every later call folds its batch in with the current topics (transform),
        runs `sweeps` sweeps in which the earlier batches take part as frozen rows (nmf(frozen=): their W no longer moves,
        they enter every T-row update through their sums `self.frozen_`, scaled by `decay` in (0, 1] first), and absorbs the
        batch.  self.W is the W of the last batch; with handle_tfidf the idf of the first batch is used throughout, as
        transform does.  The options nmf(frozen=) refuses in nmf_kwargs are refused here."""
        assert _all_nonnegative(X), 'X must be non-negative'
        sweeps = int(sweeps)
        if sweeps < 1:
            raise ValueError('sweeps must be >= 1')
        if not 0.0 < decay <= 1.0:
            raise ValueError('decay %r is outside (0, 1]' % (decay,))
        flags = dict(max_iter=sweeps, max_time=7200, project_W_each_iter=False, w_row_sum=1.0, project_T_each_iter=True,
                     t_row_sum=1.0, do_final_project_W=self.do_final_project_W, reg_w_l1=self.wr1, reg_w_l2=self.wr2,
                     reg_t_l1=self.tr1, reg_t_l2=self.tr2, random_state=self.random_state)
        if getattr(self, 'frozen_', None) is None:
            W_in, T_in = self._warm_start()
            soln = _nmf(X, self.k, W_in=W_in, T_in=T_in, frozen=True, **dict(self._preprocess_kwargs(), **self.nmf_kwargs), **flags)
            if self.handle_tfidf:
                self.idf = soln['idf']
        else:
            W_in = self.transform(X)
            kw = dict(self._preprocess_kwargs(idf=self.idf if self.handle_tfidf else None), **self.nmf_kwargs)
            soln = _nmf(X, self.k, W_in=W_in, T_in=self.T, frozen=self.frozen_.decay(decay), **kw, **flags)
        self.frozen_ = soln.pop('frozen')
        self._keep(soln)
        return self

    def transform(self, Xnew):
        """express Xnew in the fitted topics (4 sweeps over W with T fixed)"""
        soln = _nmf(Xnew, self.k, max_iter=4, max_time=7200, project_W_each_iter=False, w_row_sum=1.0,
                    t_row_sum=1.0, T_in=self.T, do_final_project_W=self.do_final_project_W, fix_T=True,
                    reg_w_l1=self.wr1, reg_w_l2=self.wr2, reg_t_l1=self.tr1, reg_t_l2=self.tr2,
                    random_state=self.random_state,
                    **self._preprocess_kwargs(idf=self.idf if self.handle_tfidf else None),
                    # the storage options of nmf_kwargs the fold-in follows: X kept as CSR on the device, and a float16 or uint8
                    # store (without it the fold-in would upload the new rows at 8 bytes per entry)
                    **({'sparse_X': self.nmf_kwargs['sparse_X']} if 'sparse_X' in self.nmf_kwargs else {}),
                    # ... and with it the uniform rows that keep new documents without a term on the device route
                    **({'uniform_rows': self.nmf_kwargs['uniform_rows']} if 'uniform_rows' in self.nmf_kwargs else {}),
                    **({'dtype': self._read_only_storage()} if self._read_only_storage() is not None else {}))
        return soln['W']

    def _read_only_storage(self):
        """np.float16 or np.uint8 where nmf_kwargs asks for one of the two stores of an X that is only read, else None"""
        dt = self.nmf_kwargs.get('dtype')
        for store in (np.float16, np.uint8):
            if dt is not None and np.dtype(dt) == store:
                return store
        return None

    def constrained_transform(self, X):
        return self.transform(X)

    def score(self, X, y=None):
        """R^2 of the reconstruction of new documents (sklearn_interface.py:339-345); the residual sum of squares
        is taken on the device (rri_objective) instead of through an n x d product on the host"""
        if isinstance(X, DeviceCorpus):
            raise TypeError('score() centres X on the host: it takes an array, not a DeviceCorpus (corpus.to_scipy().toarray())')
        sst = ((X - np.mean(X, axis=0)) ** 2).sum()
        W = self.transform(X)
        calc = _nmf_module.TrueObjComputer(np.asarray(X), W, self.T, 0, 0, 0, 0, None, None)
        sse = 2.0 * calc.true_objective()
        return 1 - sse / sst

    def top_words(self, n_words=10):
        """The n_words heaviest words of every topic: (k, n_words) int32 columns of T.  A topic's words are ordered by the larger
        entry of its row of T first and, among equal entries, by the smaller column (the order of rri_topn.hpp); only positive
        entries qualify, and the slots after them hold -1.  Taken on the host -- T is k x d --, from a sparsified T as well."""
        if np.ndim(self.T) != 2:
            raise ValueError('the estimator is not fitted: it has no T')
        n_words = int(n_words)
        if n_words < 1:
            raise ValueError('n_words must be a positive integer')
        T = self.T.tocsr() if sp.issparse(self.T) else np.asarray(self.T)
        out = np.full((T.shape[0], n_words), -1, dtype=np.int32)
        for t in range(T.shape[0]):
            row = T[t].toarray().ravel() if sp.issparse(T) else T[t]
            cand = np.flatnonzero(row > 0)                            # ascending columns; NaN does not qualify
            best = cand[np.argsort(-row[cand], kind='stable')][:n_words]      # stable: equal entries keep the smaller column first
            out[t, :best.size] = best
        return out

    def coherence(self, X, n_words=10, measure='npmi', eps=1.0, words=None):
        """Topic coherence over document co-occurrence in the corpus X (n' x d, any number of documents): a dict.

        A word OCCURS in a document where X has a stored non-zero: presence is taken from X as given, without tf-idf or
        normalisation (an idf of 0 would erase a word).  X is scipy sparse, or dense -- which is converted to CSR on the host
        first, the slow way in --, or a DeviceCorpus, which is counted where it lives: no canonical copy on the host and no upload,
        the same counts.  `words` ((g, M), -1 for an empty slot, M <= 32) overrides top_words(n_words).  The document
        frequencies D_a and co-document frequencies D_ab of each topic's words are counted on the device
        (rri_cooccurrence_counts); there is no host route for them: without a GPU the call raises RRIHipUnavailable.

        The measures are taken on the host in float64.  With N documents, over the pairs of slots a < b in top-word order:
          'umass'  log((D_ab + eps) / D_a);                     undefined when D_a = 0
          'pmi'    log((D_ab + eps) N / (D_a D_b));             undefined when D_a D_b = 0
          'npmi'   -1 when D_ab = 0, 1 when D_ab = N, else log(p_ab / (p_a p_b)) / (-log p_ab) with p = D / N;
                   undefined when D_a D_b = 0; eps is not used
        A topic's figure is the mean over its defined pairs (pairs with an empty slot are no pairs).

        Returns measure, per_topic (NaN for a topic without a defined pair), mean (the nanmean of per_topic), words, df (g, M),
        codf (g, M, M), documents (N), pairs_undefined (per topic) and diversity: the number of distinct words among all non-empty
        slots divided by the number of those slots."""
        if measure not in ('umass', 'pmi', 'npmi'):
            raise ValueError("measure must be 'umass', 'pmi' or 'npmi', not %r" % (measure,))
        if np.ndim(self.T) != 2:
            raise ValueError('the estimator is not fitted: it has no T')
        d = np.shape(self.T)[1]
        A = X if isinstance(X, DeviceCorpus) else X.tocsr() if sp.issparse(X) else sp.csr_matrix(np.asarray(X))
        if A.shape[1] != d:
            raise ValueError('X must have the %d columns of T, not %d' % (d, A.shape[1]))
        words = self.top_words(n_words) if words is None else np.array(words, dtype=np.int32, ndmin=2)
        if words.ndim != 2:
            raise ValueError('words must be a (groups, words per group) array')
        eng = RRIEngine(1, 1, 1, dtype=np.float64, weighted=False,
                        device=A.device if isinstance(A, DeviceCorpus) else self.nmf_kwargs.get('device', 0))
        try:        # the handle gives the device and the stream: it holds nothing of the corpus's size
            df, codf = eng.cooccurrence_counts(A, words)
        finally:
            eng.close()
        N = int(A.shape[0])
        a, b = np.triu_indices(words.shape[1], 1)
        is_pair = (words[:, a] >= 0) & (words[:, b] >= 0)
        Da, Db, Dab = (np.asarray(v, dtype=np.float64) for v in (df[:, a], df[:, b], codf[:, a, b]))
        with np.errstate(divide='ignore', invalid='ignore'):
            if measure == 'umass':
                defined = is_pair & (Da > 0)
                val = np.log((Dab + eps) / Da)
            elif measure == 'pmi':
                defined = is_pair & (Da * Db > 0)
                val = np.log((Dab + eps) * N / (Da * Db))
            else:
                defined = is_pair & (Da * Db > 0)
                val = np.log((Dab / N) / ((Da / N) * (Db / N))) / -np.log(Dab / N)
                val = np.where(Dab == 0, -1.0, np.where(Dab == N, 1.0, val))
            count = defined.sum(axis=1)
            per_topic = np.where(count > 0, np.where(defined, val, 0.0).sum(axis=1) / count, np.nan)
        used = words[words >= 0]
        return {'measure': measure, 'per_topic': per_topic,
                'mean': float(np.nanmean(per_topic)) if np.any(count > 0) else float('nan'),
                'words': words, 'df': df, 'codf': codf, 'documents': N,
                'pairs_undefined': (is_pair & ~defined).sum(axis=1),
                'diversity': float(np.unique(used).size) / used.size if used.size else float('nan')}

    def log_likelihood(self, X, W=None, floor=1e-12):
        """The log-likelihood of the term counts X (n' x d, any number of documents) under the fitted topics: a dict.

        Document i is scored under the distribution p_i = W[i, :] T / Z_i over the dictionary, Z_i = sum_t W[i, t] sum_j T[t, j]
        being formed on the host so that every row of W T sums to one (a fitted model has Z_i = 1 up to rounding; a row with
        Z_i == 0 is left as it is, so all its entries are floored).  W is self.transform(X) when None, else the given n' x k
        weights, and no fold-in runs.  X is scipy sparse, or dense -- which is converted to CSR on the host first, the slow way
        in; its stored values are the counts as given (no tf-idf, no normalisation), finite and >= 0.  The sums
        sum_j X[i, j] log(max(p_ij, floor)) over the stored entries are taken on the device (rri_entries_loglik), so nothing of
        size n' x d exists anywhere; there is no host route for them: without a GPU the call raises RRIHipUnavailable.
        X may also be a DeviceCorpus: its entries are scored where they live (the same bits as for X.to_scipy()); one that holds
        negative values is refused.  With W=None the fold-in needs the matrix on the host, so the corpus is DOWNLOADED
        (X.to_scipy()) for it: pass W to download nothing.

        Returns per_document (n',), tokens (n',: the sum of a document's counts), floored (n',: its entries with a positive
        count whose p lies below floor), log_likelihood (the sum of per_document), per_token (that over the sum of tokens),
        perplexity = exp(-per_token), floor and documents (n').  Without any token per_token and perplexity are NaN."""
        if np.ndim(self.T) != 2:
            raise ValueError('the estimator is not fitted: it has no T')
        k, d = np.shape(self.T)
        A = X if isinstance(X, DeviceCorpus) else X.tocsr() if sp.issparse(X) else sp.csr_matrix(np.asarray(X))
        if A.shape[1] != d:
            raise ValueError('X must have the %d columns of T, not %d' % (d, A.shape[1]))
        if W is None:
            W = self.transform(X.to_scipy() if isinstance(X, DeviceCorpus) else X)
        W = W.toarray() if sp.issparse(W) else np.asarray(W, dtype=np.float64)
        if W.shape != (A.shape[0], k):
            raise ValueError('W must be %r, one row per document of X, not %r' % ((A.shape[0], k), W.shape))
        T = self.T.toarray() if sp.issparse(self.T) else np.asarray(self.T, dtype=np.float64)
        Z = W.dot(T.sum(axis=1))
        W = W / np.where(Z == 0, 1.0, Z)[:, None]
        n = int(A.shape[0])
        if n == 0:
            ll, mass, floored = np.zeros(0), np.zeros(0), np.zeros(0, dtype=np.int64)
        else:
            eng = RRIEngine(n, d, k, dtype=np.float64, device=A.device if isinstance(A, DeviceCorpus) else self.nmf_kwargs.get('device', 0))
            try:        # a factors-only handle: it holds W and T and nothing of the corpus's size
                eng.set_W(W)
                eng.set_T(T)
                ll, mass, floored = eng.entries_loglik(None, A, floor)
            finally:
                eng.close()
        total, tokens = float(ll.sum()), float(mass.sum())
        per_token = total / tokens if tokens > 0 else float('nan')
        return {'per_document': ll, 'tokens': mass, 'floored': floored, 'log_likelihood': total, 'per_token': per_token,
                'perplexity': float(np.exp(-per_token)), 'floor': float(floor), 'documents': n}

    def perplexity(self, X, observed=None, floor=1e-12):
        """exp(-log-likelihood per token) of the counts X under the fitted topics: log_likelihood(X, W, floor)['perplexity'] with
        W = self.transform(observed if observed is not None else X).  With `observed` (n' x d, the same documents) this is document
        completion: fold in on one part of each document's tokens and score the other (split_counts makes the two parts).  A
        model that spreads every document evenly over the dictionary has perplexity d.  X may be a DeviceCorpus: with a scipy
        `observed` nothing is downloaded; without `observed` the fold-in downloads the corpus (X.to_scipy())."""
        seen = observed if observed is not None else X
        return self.log_likelihood(X, W=self.transform(seen.to_scipy() if isinstance(seen, DeviceCorpus) else seen), floor=floor)['perplexity']


def split_counts(X, held_out=0.5, random_state=0):
    """Thin the integer counts X (n x d, scipy sparse or dense) binomially into (observed, held), two CSR matrices with
    observed + held == X: every token of a stored count goes to `held` with probability held_out, independently, so
    held = binomial(x, held_out) entry by entry (vectorised over the stored values, on the host).  For document completion:
    NMF_TM_Estimator.perplexity(held, observed=observed).  Explicit zeros are dropped from both parts.  ValueError for values
    that are negative or not whole numbers, or for a held_out outside (0, 1).

    A DeviceCorpus is split where it lives: X.split_counts(held_out, random_state) returns two corpora on its device and nothing
    of the corpus's size visits the host.  The two routes use different generators -- numpy's binomial here, a counter-based
    Philox4x32-10 there --, so the same seed gives a different split on the two routes; both are the same binomial thinning and
    equally valid, and each is reproducible from its seed."""
    if isinstance(X, DeviceCorpus):
        return X.split_counts(held_out=held_out, random_state=random_state)
    if not 0.0 < held_out < 1.0:
        raise ValueError('held_out must lie inside (0, 1), not %r' % (held_out,))
    A = sp.csr_matrix(X, copy=True)
    A.sum_duplicates()
    x = np.asarray(A.data)
    if x.size and (not np.all(np.isfinite(x)) or np.any(x < 0) or np.any(x != np.floor(x))):
        raise ValueError('split_counts needs counts: non-negative whole numbers')
    rs = random_state if isinstance(random_state, np.random.RandomState) else np.random.RandomState(random_state)
    h = rs.binomial(x.astype(np.int64), held_out).astype(A.dtype)
    held = sp.csr_matrix((h, A.indices.copy(), A.indptr.copy()), shape=A.shape)
    observed = sp.csr_matrix((x - h, A.indices.copy(), A.indptr.copy()), shape=A.shape)
    held.eliminate_zeros()
    observed.eliminate_zeros()
    return observed, held


def split_entries(X, held_out=0.05, random_state=0):
    """Split the stored entries of X (n x d, scipy sparse or dense) into (observed, held), two CSR matrices: every entry goes,
    whole and with its value as it is, to `held` with probability held_out and to `observed` otherwise -- the split of observed
    ratings into a training and a held-out part.  Values may be negative or fractional; duplicates are summed and explicit zeros
    dropped first, the patterns of the two parts are disjoint and their union is X's.  ValueError for a held_out outside (0, 1).

    A DeviceCorpus is split where it lives: X.split_entries(held_out, random_state) returns two corpora on its device.  The two
    routes use different generators -- one uniform draw per stored entry from numpy's RandomState here, a counter-based
    Philox4x32-10 keyed by (row, column) there --, so the same seed gives a different split on the two routes; both send every
    entry to `held` independently with the same probability and are equally valid, and each is reproducible from its seed."""
    if isinstance(X, DeviceCorpus):
        return X.split_entries(held_out=held_out, random_state=random_state)
    if not 0.0 < held_out < 1.0:
        raise ValueError('held_out must lie inside (0, 1), not %r' % (held_out,))
    A = sp.csr_matrix(X, copy=True)
    A.sum_duplicates()
    A.eliminate_zeros()
    A.sort_indices()
    rs = random_state if isinstance(random_state, np.random.RandomState) else np.random.RandomState(random_state)
    to_held = rs.random_sample(A.nnz) < held_out
    rows = np.repeat(np.arange(A.shape[0]), np.diff(A.indptr))
    parts = []
    for take in (~to_held, to_held):
        indptr = np.concatenate(([0], np.cumsum(np.bincount(rows[take], minlength=A.shape[0])))).astype(A.indptr.dtype)
        parts.append(sp.csr_matrix((A.data[take], A.indices[take], indptr), shape=A.shape))
    return parts[0], parts[1]


def split_rows(X, n_held=None, held_out=None, min_observed=1, random_state=0):
    """Split the stored entries of X (n x d, scipy sparse or dense) into (observed, held), two CSR matrices, row by row: every row
    gives up an exact number of its entries, whole and with their values as they are -- leave-k-out with n_held=k, or a share of
    every row with held_out (exactly one of the two is given).  A row of L entries gives up h = min(want, max(L - min_observed, 0))
    of them, want being n_held or floor(held_out L + 0.5): a row keeps at least min_observed entries and gives up fewer, or none,
    where it is short.  Duplicates are summed and explicit zeros dropped first, the patterns of the two parts are disjoint and their
    union is X's.  ValueError for both modes or neither, n_held below 1, a held_out outside (0, 1] and a negative min_observed.

    A DeviceCorpus is split where it lives: X.split_rows(n_held, held_out, min_observed, random_state) returns two corpora on its
    device.  The quota of a row is the same function on both routes; which entries a row gives up is not: the two routes use
    different generators -- numpy's RandomState.choice without replacement here, row after row; the h smallest keys of a
    counter-based Philox4x32-10 keyed by (row, column) there --, so the same seed gives a different split on the two routes;
    both choose the h entries of a row uniformly among its subsets of that size and are equally valid, and each is reproducible from
    its seed."""
    if isinstance(X, DeviceCorpus):
        return X.split_rows(n_held=n_held, held_out=held_out, min_observed=min_observed, random_state=random_state)
    n_held, fraction, min_observed = DeviceCorpus._split_rows_request(n_held, held_out, min_observed)
    A = sp.csr_matrix(X, copy=True)
    A.sum_duplicates()
    A.eliminate_zeros()
    A.sort_indices()
    rs = random_state if isinstance(random_state, np.random.RandomState) else np.random.RandomState(random_state)
    lengths = np.diff(A.indptr).astype(np.int64)
    quota = DeviceCorpus._split_rows_quota(lengths, n_held, fraction, min_observed)
    rows = np.repeat(np.arange(A.shape[0]), lengths)
    to_held = np.zeros(A.nnz, dtype=bool)
    for r in np.flatnonzero(quota > 0):          # a choice per row: linear in the entries, where a sort of all draws is not
        lo, L, h = int(A.indptr[r]), int(lengths[r]), int(quota[r])
        to_held[lo + rs.choice(L, size=h, replace=False) if h < L else slice(lo, lo + L)] = True
    parts = []
    for take in (~to_held, to_held):
        indptr = np.concatenate(([0], np.cumsum(np.bincount(rows[take], minlength=A.shape[0])))).astype(A.indptr.dtype)
        parts.append(sp.csr_matrix((A.data[take], A.indices[take], indptr), shape=A.shape))
    return parts[0], parts[1]
