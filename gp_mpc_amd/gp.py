"""`GP`: host-side mirror of the reference's `gp_mpc.GP` class (gp_class.py:20-861) for the hot path.

Same constructor, method names, argument meaning and error behaviour as the reference, so that a
caller such as `mpc_class.MPC` (mpc_class.py:167,234,412-413,596) can use it unchanged; all GP
arithmetic runs in the HIP kernels behind the C ABI (include/gpmpc.h) -- there is no CPU path.
Differences that are deliberate are marked "DIFF".

Standardisation stays on the host exactly as in the reference: `predict` standardises x and u,
calls the (device) predictor in the GP's own units and un-standardises the MEAN only
(gp_class.py:245-263); `discrete_linearize` returns Jacobians in standardised coordinates
(gp_class.py:647-661).
"""
from __future__ import annotations

import json
import os

import numpy as np

from . import _lib
from .train import train_gp

METHODS = ('ME', 'TA', 'EM', 'old_ME', 'old_TA')


def _listify(v):
    """numpy arrays -> nested lists, recursively through dicts (json.dump input)."""
    if isinstance(v, dict):
        return {k: _listify(x) for k, x in v.items()}
    if isinstance(v, np.ndarray):
        return v.tolist()
    return v


class GP:
    def __init__(self, X, Y, mean_func="zero", gp_method="TA",
                 optimizer_opts=None, hyper=None, normalize=True, multistart=1,
                 xlb=None, xub=None, ulb=None, uub=None, meta=None,
                 optimize_nummeric=True, device=0, lib=None, predict_adds_mean=False, optimizer='native'):
        """Initialize and optimize GP model (gp_class.py:21-75).

        Extra arguments: `device` (GPU ordinal), `lib` (a loaded `GpmpcLib`; default: the in-tree
        libgpmpc_hip.so, raising if it is missing) and `predict_adds_mean`: the reference builds its predictor
        WITHOUT the mean function (`build_gp(...)` is called with its default meanFunc='zero', gp_class.py:68-71),
        so a model trained with mean_func != 'zero' predicts ks^T alpha only; that is the default here too.
        `optimizer`: 'native' (default) or 'scipy', see gp_mpc_amd.train.train_gp.
        True gives build_gp(..., meanFunc=mean_func) (gp_functions.py:131,135): mean(z) = ks^T alpha + m(z)."""
        self._lib = lib if lib is not None else _lib.get_lib()
        self._device = device
        X = np.array(X, dtype=np.float64).copy()
        Y = np.array(Y, dtype=np.float64).copy()
        self.__X = X
        self.__Y = Y
        self.__Ny = Y.shape[1]
        self.__Nx = X.shape[1]
        self.__N = X.shape[0]
        self.__Nu = self.__Nx - self.__Ny
        self.__gp_method = gp_method
        self.__mean_func = mean_func
        self.__normalize = normalize
        self._predict_adds_mean = bool(predict_adds_mean)
        self._h = None
        self._sparse = False                  # True on what GP.sparse returns: a FITC model, predict-only
        self._check_mean_func(mean_func)

        if meta is not None:
            self.__meanY = np.array(meta['meanY'])
            self.__stdY = np.array(meta['stdY'])
            self.__meanZ = np.array(meta['meanZ'])
            self.__stdZ = np.array(meta['stdZ'])
            self.__meanX = np.array(meta['meanX'])
            self.__stdX = np.array(meta['stdX'])
            self.__meanU = np.array(meta['meanU'])
            self.__stdU = np.array(meta['stdU'])
        if xlb is not None:
            self.__xlb, self.__xub = np.array(xlb), np.array(xub)
            self.__ulb, self.__uub = np.array(ulb), np.array(uub)

        if hyper is None:
            self.optimize(X=X, Y=Y, opts=optimizer_opts, mean_func=mean_func,
                          xlb=xlb, xub=xub, ulb=ulb, uub=uub,
                          multistart=multistart, normalize=normalize,
                          optimize_nummeric=optimize_nummeric, optimizer=optimizer)
        else:
            # load_model branch (gp_class.py:58-66): stored X is already standardised
            self.__hyper = np.array(hyper['hyper'], dtype=np.float64)
            self.__hyper_length_scales = self.__hyper[:, :self.__Nx]
            self.__hyper_signal_variance = self.__hyper[:, self.__Nx] ** 2
            self.__hyper_noise_variance = self.__hyper[:, self.__Nx + 1] ** 2
            self.__hyper_mean = self.__hyper[:, (self.__Nx + 1):]
            self._new_handle()
            self._h.set_mean_func(mean_func, self._predict_adds_mean)
            self._h.set_factors(self.__hyper, np.array(hyper['chol'], dtype=np.float64),
                                None if hyper.get('alpha') is None else np.array(hyper['alpha'], dtype=np.float64),
                                None if hyper.get('invK') is None else np.array(hyper['invK'], dtype=np.float64))
        self.set_method(gp_method)

    # ------------------------------------------------------------------ internals
    @staticmethod
    def _check_mean_func(mean_func):
        if mean_func not in ('zero', 'const', 'linear', 'polynomial'):
            raise NameError('No mean function called: ' + str(mean_func))      # gp_functions.py:67

    def _refuse_sparse(self, what):
        if self._sparse:
            raise RuntimeError(what + ': this object is a FITC sparse model (GP.sparse) and is predict-only; '
                               'change the data or the hyper-parameters on the full model and call sparse() again')

    def _new_handle(self):
        if self._h is not None:
            self._h.close()
        self._h = _lib.Handle(self._lib, self.__X, self.__Y, device=self._device)

    def _refit(self, want_invK=False):
        self._new_handle()
        self._h.set_mean_func(self.__mean_func, self._predict_adds_mean)
        self._h.fit(self.__hyper, want_invK=want_invK)

    @property
    def handle(self):
        """The C-ABI handle (for batched / device-pointer use)."""
        return self._h

    # ------------------------------------------------------------------ training
    def optimize(self, X=None, Y=None, opts=None, mean_func='zero',
                 xlb=None, xub=None, ulb=None, uub=None,
                 multistart=1, normalize=True, warm_start=False,
                 optimize_nummeric=True, random_restarts=False, seed=1234, gradient='analytic', optimizer='native'):
        """Optimize hyper-parameters (gp_class.py:78-142).  DIFF: both of the reference's optimiser
        back-ends (scipy SLSQP with finite differences / CasADi+IPOPT) are replaced by one driver
        (`gp_mpc_amd.train.train_gp`) that evaluates the NLL and its analytic gradient on the GPU;
        `optimize_nummeric` selects the reference's bound/initialisation convention of the
        corresponding path (True: optimize.py:434-449, False: optimize.py:207-229)."""
        self._refuse_sparse('optimize')
        self._check_mean_func(mean_func)
        self.__mean_func = mean_func
        self.__normalize = normalize

        if normalize and X is not None:
            self.__xlb = np.array(xlb)
            self.__xub = np.array(xub)
            self.__ulb = np.array(ulb)
            self.__uub = np.array(uub)
            self.__meanY = np.mean(Y, 0)
            self.__stdY = np.std(Y, 0)
            self.__meanZ = np.mean(X, 0)
            self.__stdZ = np.std(X, 0)
            self.__meanX = np.mean(X[:, :self.__Ny], 0)
            self.__stdX = np.std(X[:, :self.__Ny], 0)
            self.__meanU = np.mean(X[:, self.__Ny:], 0)
            self.__stdU = np.std(X[:, self.__Ny:], 0)

        if X is not None:
            X = np.array(X, dtype=np.float64).copy()
            self.__X = self.standardize(X, self.__meanZ, self.__stdZ) if normalize else X.copy()
        if Y is not None:
            Y = np.array(Y, dtype=np.float64).copy()
            self.__Y = self.standardize(Y, self.__meanY, self.__stdY) if (normalize and X is not None) else Y.copy()
        self.__N = self.__X.shape[0]

        hyp_init = self.__hyper if warm_start else None
        self._new_handle()
        opt = train_gp(self._h, self.__X, self.__Y, multistart=multistart, hyper_init=hyp_init,
                       optimizer_opts=opts, numpy_path_conventions=optimize_nummeric,
                       random_restarts=random_restarts, seed=seed, gradient=gradient,
                       mean_func=mean_func, predict_adds_mean=self._predict_adds_mean, optimizer=optimizer)
        self.__hyper = opt['hyper']
        self.__lam_x = opt['lam_x']
        self.__hyper_length_scales = self.__hyper[:, :self.__Nx]
        self.__hyper_signal_variance = self.__hyper[:, self.__Nx] ** 2
        self.__hyper_noise_variance = self.__hyper[:, self.__Nx + 1] ** 2
        self.__hyper_mean = self.__hyper[:, (self.__Nx + 1):]      # off-by-one slice kept (gp_class.py:142)
        self.train_info = opt

    # ------------------------------------------------------------------ validation
    def validate(self, X_test, Y_test, verbose=True):
        """gp_class.py:145-190: SMSE (divides by std, :166) and MNLP; all test rows in ONE batched
        device call instead of the reference's per-row loop."""
        Y_test = np.array(Y_test, dtype=np.float64).copy()
        X_test = np.array(X_test, dtype=np.float64).copy()
        if self.__normalize:
            Y_test = self.standardize(Y_test, self.__meanY, self.__stdY)
            X_test = self.standardize(X_test, self.__meanZ, self.__stdZ)
        N, Ny = Y_test.shape
        mean, var = self._h.predict_mean_var(X_test)
        var = var + self.noise_variance()
        loss = np.sum((Y_test - mean) ** 2, axis=0) / N
        NLP = np.sum(0.5 * np.log(2 * np.pi * var) + (Y_test - mean) ** 2 / (2 * var), axis=0)
        SMSE = loss / np.std(Y_test, 0)
        MNLP = NLP / N
        if verbose:
            print('\n________________________________________')
            print('# Validation of GP model ')
            print('----------------------------------------')
            print('* Num training samples: ' + str(self.__N))
            print('* Num test samples: ' + str(N))
            for name, arr in (('Mean squared error', loss), ('Standardized mean squared error', SMSE),
                              ('Mean Negative log Probability', MNLP)):
                print('----------------------------------------')
                print('* %s:' % name)
                for i in range(Ny):
                    print('\t- State %d: %f' % (i + 1, arr[i]))
            print('----------------------------------------\n')
        self.__SMSE = np.max(SMSE)
        return np.array(SMSE).flatten(), np.array(MNLP).flatten()

    # ------------------------------------------------------------------ prediction
    def set_method(self, gp_method='TA'):
        """Select which GP function to use (gp_class.py:193-242).  DIFF: strings are compared with
        `==` (the reference's `is` only works through CPython string interning)."""
        if gp_method not in METHODS:
            raise NameError('No GP method called: ' + str(gp_method))          # gp_class.py:237
        self.__gp_method = gp_method

    def predict(self, x, u, cov):
        """Predict future state (gp_class.py:245-263): x (Ny), u (Nu), cov of z=[x,u] (Nx x Nx)
        -> mean (Ny x 1), cov (Ny x Ny, standardised units)."""
        x = np.asarray(x, dtype=np.float64).reshape(-1)
        u = np.asarray(u, dtype=np.float64).reshape(-1)
        if self.__normalize:
            x = self.standardize(x, self.__meanX, self.__stdX)
            u = self.standardize(u, self.__meanU, self.__stdU)
        z = np.concatenate([x, u]).reshape(1, self.__Nx)
        S = np.asarray(cov, dtype=np.float64).reshape(1, self.__Nx, self.__Nx)
        mean, c = self._h.predict(self.__gp_method, z, S)
        mean = mean[0]
        if self.__normalize:
            mean = self.inverse_mean(mean, self.__meanY, self.__stdY)
        return mean.reshape(self.__Ny, 1), c[0]

    def predict_derivatives(self, x, u, cov, values=True):
        """`predict` plus the exact first derivatives of both outputs with respect to all three inputs,
        for the 'ME', 'TA' and 'EM' methods -- what a casadi Callback standing in for `__predict`
        (gp_class.py:212-224) must provide through `get_jacobian`; the reference gets them from CasADi's
        AD of build_gp / build_TA_cov / gp_exact_moment (gp_functions.py:114-173,344-418).  One device call
        (`gpmpc_predict_sens`: mean, var, J, d2 mean/dz2, d var/dz, closed-form assembly here; 'EM':
        `gpmpc_predict_em_sens`, the Jacobians themselves).

        Returns (mean[Ny,1], cov[Ny,Ny], D) with D a dict of
          'dmean_dx' [Ny,Ny], 'dmean_du' [Ny,Nu], 'dmean_dcov' [Ny,Nx,Nx] (zero for ME / TA),
          'dcov_dx' [Ny,Ny,Ny], 'dcov_du' [Ny,Ny,Nu], 'dcov_dcov' [Ny,Ny,Nx,Nx],
        all with respect to the RAW x, u (the chain rule through the standardisation is applied; cov
        stays in standardised units exactly as `predict` returns it, gp_class.py:262).
        values=False (a Jacobian callback): the returned cov is None for 'EM' -- its pair sums are a quarter
        of the device call and the derivatives do not need them."""
        if self.__gp_method not in ('ME', 'TA', 'EM'):
            raise NotImplementedError("analytic derivatives exist for 'ME', 'TA' and 'EM'; use finite differences of "
                                      "GP.predict for '%s'" % self.__gp_method)
        Ny, Nx, Nu = self.__Ny, self.__Nx, self.__Nu
        x = np.asarray(x, dtype=np.float64).reshape(-1)
        u = np.asarray(u, dtype=np.float64).reshape(-1)
        if self.__normalize:
            x = self.standardize(x, self.__meanX, self.__stdX)
            u = self.standardize(u, self.__meanU, self.__stdU)
        z = np.concatenate([x, u]).reshape(1, Nx)
        S = np.asarray(cov, dtype=np.float64).reshape(Nx, Nx)
        if self.__gp_method == 'EM':
            mean, c, dmean, dmS, dcz, dcS = (None if a is None else a[0]
                                             for a in self._h.predict_em_sens(z, S.reshape(1, Nx, Nx), want_cov=values))
        else:
            mean, var, J, Hm, dvar = (a[0] for a in self._h.predict_sens(z))
            c = np.diag(var)
            dcz = np.zeros((Ny, Ny, Nx))
            dcz[np.arange(Ny), np.arange(Ny)] = dvar                      # d diag(var) / dz
            dcS = np.zeros((Ny, Ny, Nx, Nx))
            dmS = np.zeros((Ny, Nx, Nx))
            if self.__gp_method == 'TA':                                  # cov = diag(var) + J S J^T
                c = c + J @ S @ J.T
                dcz += np.einsum('adp,de,ce->acp', Hm, S, J) + np.einsum('ad,de,cep->acp', J, S, Hm)
                dcS = np.einsum('ad,ce->acde', J, J)
            dmean = J.copy()
        if self.__normalize:
            mean = self.inverse_mean(mean, self.__meanY, self.__stdY)
            sz = np.concatenate([np.atleast_1d(self.__stdX), np.atleast_1d(self.__stdU)])
            dmean = dmean * np.atleast_1d(self.__stdY)[:, None] / sz[None, :]
            dmS = dmS * np.atleast_1d(self.__stdY)[:, None, None]
            dcz = dcz / sz[None, None, :]
        D = {'dmean_dx': dmean[:, :Ny], 'dmean_du': dmean[:, Ny:], 'dmean_dcov': dmS,
             'dcov_dx': dcz[:, :, :Ny], 'dcov_du': dcz[:, :, Ny:], 'dcov_dcov': dcS}
        return mean.reshape(Ny, 1), c, D

    def predict_derivatives_batch(self, X, U, C, values=True):
        """`predict_derivatives` for B shooting nodes in ONE device call (the pattern an NLP evaluation produces: IPOPT
        asks for the Jacobian of all Nt continuity constraints at once, mpc_class.py:361-423).  X[B,Ny], U[B,Nu],
        C[B,Nx,Nx] -> mean[B,Ny], cov[B,Ny,Ny] (None for 'EM' with values=False) and D as in `predict_derivatives` with
        a leading node axis.  'ME' / 'TA' / 'EM' only."""
        if self.__gp_method not in ('ME', 'TA', 'EM'):
            raise NotImplementedError("analytic derivatives exist for 'ME', 'TA' and 'EM'")
        Ny, Nx, Nu = self.__Ny, self.__Nx, self.__Nu
        X = np.asarray(X, dtype=np.float64).reshape(-1, Ny)
        U = np.asarray(U, dtype=np.float64).reshape(-1, Nu)
        B = X.shape[0]
        if self.__normalize:
            X = self.standardize(X, self.__meanX, self.__stdX)
            U = self.standardize(U, self.__meanU, self.__stdU)
        Z = np.concatenate([X, U], axis=1)
        S = np.asarray(C, dtype=np.float64).reshape(B, Nx, Nx)
        if self.__gp_method == 'EM':
            mean, c, dmean, dmS, dcz, dcS = self._h.predict_em_sens(Z, S, want_cov=values)
        else:
            mean, var, J, Hm, dvar = self._h.predict_sens(Z)
            ia = np.arange(Ny)
            c = np.zeros((B, Ny, Ny))
            c[:, ia, ia] = var
            dcz = np.zeros((B, Ny, Ny, Nx))
            dcz[:, ia, ia] = dvar
            dcS = np.zeros((B, Ny, Ny, Nx, Nx))
            dmS = np.zeros((B, Ny, Nx, Nx))
            if self.__gp_method == 'TA':
                c = c + np.einsum('bad,bde,bce->bac', J, S, J)
                dcz += np.einsum('badp,bde,bce->bacp', Hm, S, J) + np.einsum('bad,bde,bcep->bacp', J, S, Hm)
                dcS = np.einsum('bad,bce->bacde', J, J)
            dmean = J.copy()
        if self.__normalize:
            mean = self.inverse_mean(mean, self.__meanY, self.__stdY)
            sz = np.concatenate([np.atleast_1d(self.__stdX), np.atleast_1d(self.__stdU)])
            dmean = dmean * np.atleast_1d(self.__stdY)[None, :, None] / sz[None, None, :]
            dmS = dmS * np.atleast_1d(self.__stdY)[None, :, None, None]
            dcz = dcz / sz[None, None, None, :]
        D = {'dmean_dx': dmean[:, :, :Ny], 'dmean_du': dmean[:, :, Ny:], 'dmean_dcov': dmS,
             'dcov_dx': dcz[:, :, :, :Ny], 'dcov_du': dcz[:, :, :, Ny:], 'dcov_dcov': dcS}
        return mean.reshape(B, Ny), c, D

    def predict_batch(self, Z, Sigma=None, method=None, standardized=True):
        """All B inputs in one device call (the pattern MPC's Nt shooting nodes want):
        Z[B x Nx] (already standardised unless standardized=False), Sigma[B x Nx x Nx]
        -> mean[B x Ny] (un-standardised like `predict`), cov[B x Ny x Ny]."""
        Z = np.asarray(Z, dtype=np.float64).reshape(-1, self.__Nx)
        if self.__normalize and not standardized:
            Z = self.standardize(Z, self.__meanZ, self.__stdZ)
        mean, c = self._h.predict(method or self.__gp_method, Z, Sigma)
        if self.__normalize:
            mean = self.inverse_mean(mean, self.__meanY, self.__stdY)
        return mean, c

    def get_size(self):
        """(N, Ny, Nu) -- gp_class.py:266-274."""
        return self.__N, self.__Ny, self.__Nu

    def get_hyper_parameters(self):
        """gp_class.py:277-290."""
        return dict(length_scale=self.__hyper_length_scales, signal_var=self.__hyper_signal_variance,
                    noise_var=self.__hyper_noise_variance, mean=self.__hyper_mean)

    def print_hyper_parameters(self):
        """Print all hyper-parameters (what gp_class.py:293-312 reports: sizes, per output the d
        length scales, signal variance sf^2 and noise variance sn^2)."""
        rule = '-' * 40
        lines = ['', '_' * 40, '# Hyper-parameters', rule,
                 f'* Num samples: {self.__N}', f'* Ny: {self.__Ny}', f'* Nu: {self.__Nu}',
                 f'* Normalization: {self.__normalize}']
        for a in range(self.__Ny):
            lines += [rule, f'* Lengthscale:  {a}']
            lines += [f'-- l{i}: {ell}' for i, ell in enumerate(self.__hyper_length_scales[a])]
            lines += [f'* Signal variance:  {a}', f'-- sf2: {self.__hyper_signal_variance[a]}',
                      f'* Noise variance:  {a}', f'-- sn2: {self.__hyper_noise_variance[a]}']
        lines.append(rule)
        print('\n'.join(lines))

    def covSEard(self, X, Z, ell, sf2):
        """GP squared exponential kernel k(X, Z) (gp_class.py:314-350), evaluated on the device."""
        X = np.atleast_2d(np.asarray(X, dtype=np.float64))
        Z = np.atleast_2d(np.asarray(Z, dtype=np.float64))
        if X.shape[1] != Z.shape[1]:
            raise ValueError('Input dimensions are not the same! D_x=' + str(X.shape[1])
                             + ', D_z=' + str(Z.shape[1]))                      # gp_class.py:342-344
        return self._lib.kernel_matrix(X, Z, np.asarray(ell, dtype=np.float64), float(sf2), device=self._device)

    def covar(self, X_new):
        """Posterior covariance between new inputs (gp_class.py:353-381): (D x n x n) array whose
        first Ny slabs are filled, like the reference."""
        X_new = np.atleast_2d(np.asarray(X_new, dtype=np.float64))
        n, D = X_new.shape
        out = np.zeros((D, n, n))
        out[:self.__Ny] = self._h.covar(X_new)
        return out

    # ------------------------------------------------------------------ data updates
    def update_data(self, X_new, Y_new, N_new=None):
        """The reference documents its incremental update as not working (gp_class.py:384-471:
        argmin for 'max variance' :421, norm instead of norm^2 :443); `update_data_select` does what it set out to
        do, `update_data_all` appends everything."""
        self._refuse_sparse('update_data')
        raise NotImplementedError('update_data is broken in the reference (gp_class.py:384-471); '
                                  'use update_data_select (the N_new most informative points), '
                                  'update_data_all / replace_data_all')

    def update_data_select(self, X_new, Y_new=None, N_new=None, min_gain=0.0):
        """From the new observations take only the `N_new` most informative ones (default: up to all) -- what the
        reference's `update_data` intended (gp_class.py:384-471): repeatedly the point whose predictive variance, summed
        over the outputs, is largest given the model AND the points taken so far (`gpmpc_append_select`).  Differences to
        the reference's text: arg-max instead of its argmin (:421), the squared norm instead of the norm (:443), and the
        noise enters only where a taken point joins K (:440) -- the scores are the noise-free variances of `covar`.
        Selection stops early when the best score (standardised units) falls below `min_gain` (> 0).  The taken rows are
        appended like `update_data_all` does; `Y_new=None` only selects (experiment design) and changes nothing.
        Returns (indices into X_new in pick order, their scores when picked)."""
        self._refuse_sparse('update_data_select')
        X_new = np.array(X_new, dtype=np.float64).copy().reshape(-1, self.__Nx)
        if Y_new is not None:
            Y_new = np.array(Y_new, dtype=np.float64).copy().reshape(-1, self.__Ny)
        if self.__normalize:
            X_new = self.standardize(X_new, self.__meanZ, self.__stdZ)
            if Y_new is not None:
                Y_new = self.standardize(Y_new, self.__meanY, self.__stdY)
        try:
            sel, gain = self._h.append_select(X_new, Y_new, N_new, min_gain)
        finally:
            grown = self._h.N - self.__N                  # (0 for selection only and when the append was refused)
            if grown > 0:
                taken = self._h.selected[:grown]
                self.__X = np.vstack([self.__X, X_new[taken]])
                self.__Y = np.vstack([self.__Y, Y_new[taken]])
                self.__N = self.__X.shape[0]
        return sel, gain

    def _set_data_and_refit(self, X, Y):
        self.__X, self.__Y = X, Y
        self.__N = X.shape[0]
        self._refit()

    def update_data_all(self, X_new, Y_new):
        """Append all new observations and bring chol/alpha/invK up to date with the EXISTING
        hyper-parameters (gp_class.py:474-550).  The reference recomputes everything, O(N^3); here
        the factors are extended on the device (`gpmpc_append`, O(N^2 n)) -- same result to rounding."""
        self._refuse_sparse('update_data_all')
        X_new = np.array(X_new, dtype=np.float64).copy().reshape(-1, self.__Nx)
        Y_new = np.array(Y_new, dtype=np.float64).copy().reshape(-1, self.__Ny)
        if self.__normalize:
            Y_new = self.standardize(Y_new, self.__meanY, self.__stdY)
            X_new = self.standardize(X_new, self.__meanZ, self.__stdZ)
        self._h.append(X_new, Y_new)
        self.__X = np.vstack([self.__X, X_new])
        self.__Y = np.vstack([self.__Y, Y_new])
        self.__N = self.__X.shape[0]

    def remove_data(self, idx):
        """Take the training rows `idx` (distinct indices into the current data) out of the model, keep the
        hyper-parameters; the other rows keep their order.  The reference has nothing of the kind -- its only way to drop
        data is `replace_data_all` (gp_class.py:553-626), a full recomputation; here the factors are downdated on the
        device (`gpmpc_remove`, O(N^2 n)) -- same result to rounding."""
        self._refuse_sparse('remove_data')
        idx = np.asarray(idx).reshape(-1)
        n0 = self.__N
        try:
            self._h.remove(idx)
        finally:
            if self._h.N == n0 - len(idx):                # (a refused call leaves the handle's size where it was)
                keep = np.ones(n0, dtype=bool)
                keep[idx] = False
                self.__X, self.__Y = self.__X[keep], self.__Y[keep]
                self.__N = self.__X.shape[0]

    def update_data_window(self, X_new, Y_new, N_max):
        """Sliding data window: afterwards the model holds the last `N_max` rows of vstack(X, X_new), in that order, with
        the EXISTING hyper-parameters -- the fixed-budget form of `update_data_all` for a loop that keeps learning.  The
        oldest rows go first (`gpmpc_remove`, smaller factors), then the new ones are appended (`gpmpc_append`); with
        len(X_new) >= N_max it is `replace_data_all` on the last N_max new rows."""
        self._refuse_sparse('update_data_window')
        X_new = np.array(X_new, dtype=np.float64).copy().reshape(-1, self.__Nx)
        Y_new = np.array(Y_new, dtype=np.float64).copy().reshape(-1, self.__Ny)
        N_max = int(N_max)
        if N_max < 1:
            raise ValueError('update_data_window: N_max must be >= 1')
        if X_new.shape[0] >= N_max:
            return self.replace_data_all(X_new[-N_max:], Y_new[-N_max:])
        if X_new.shape[0] == 0:
            drop = self.__N - N_max
            if drop > 0:
                self.remove_data(np.arange(drop))
            return
        drop = self.__N + X_new.shape[0] - N_max
        if drop > 0:
            self.remove_data(np.arange(drop))
        self.update_data_all(X_new, Y_new)

    def replace_data_all(self, X_new, Y_new):
        """Replace the training data, keep the hyper-parameters (gp_class.py:553-626)."""
        self._refuse_sparse('replace_data_all')
        X_new = np.array(X_new, dtype=np.float64).copy()
        Y_new = np.array(Y_new, dtype=np.float64).copy()
        if self.__normalize:
            Y_new = self.standardize(Y_new, self.__meanY, self.__stdY)
            X_new = self.standardize(X_new, self.__meanZ, self.__stdZ)
        self._set_data_and_refit(X_new, Y_new)

    # ------------------------------------------------------------------ scaling helpers (gp_class.py:629-644)
    def standardize(self, Y, mean, std):
        return (Y - mean) / std

    def normalize(self, u, lb, ub):
        return (u - lb) / (ub - lb)

    def inverse_mean(self, x, mean, std):
        return (x * std) + mean

    def inverse_variance(self, variance):
        return variance * self.__stdY ** 2

    # ------------------------------------------------------------------ linearisation
    def discrete_linearize(self, x0, u0, cov0):
        """x[k+1] = A x[k] + B u[k] around (x0, u0): Jacobians of the predicted mean w.r.t. the
        standardised x and u (gp_class.py:647-661: `jac_x`, `jac_u` of `__predict`'s mean, :239-242).  For ME / TA /
        old_* that mean is the plain GP mean (analytic Jacobian on the device); for 'EM' it is the exact-moment mean,
        whose derivative with respect to the input mean comes from `gpmpc_predict_em_sens` and depends on cov0."""
        x0 = np.asarray(x0, dtype=np.float64).reshape(-1)
        u0 = np.asarray(u0, dtype=np.float64).reshape(-1)
        if self.__normalize:
            x0 = self.standardize(x0, self.__meanX, self.__stdX)
            u0 = self.standardize(u0, self.__meanU, self.__stdU)
        z = np.concatenate([x0, u0]).reshape(1, self.__Nx)
        if self.__gp_method == 'EM':
            S = np.asarray(cov0, dtype=np.float64).reshape(1, self.__Nx, self.__Nx)
            J = self._h.predict_em_sens(z, S)[2]
        else:
            _, J = self._h.mean_jac(z)
        return J[0][:, :self.__Ny].copy(), J[0][:, self.__Ny:].copy()

    def jacobian(self, x0, u0, cov0):
        """J = d mu / d x at raw (x0, u0), no standardisation (gp_class.py:664-672)."""
        z = np.concatenate([np.asarray(x0, dtype=np.float64).reshape(-1),
                            np.asarray(u0, dtype=np.float64).reshape(-1)]).reshape(1, self.__Nx)
        _, J = self._h.mean_jac(z)
        return J[0][:, :self.__Ny].copy()

    def noise_variance(self):
        return self.__hyper_noise_variance                                      # gp_class.py:675-678

    def sparse_default_inducing(self, M):
        """Indices of the M training rows `sparse` takes when no inducing points are given: row 0, then the greedy
        max-variance choice among the others with the model's hyper-parameters -- a seed model on row 0 and
        `append_select(X[1:], None, k=M-1)` on it (selection only): the pivoted-Cholesky choice, lowest index among ties."""
        M = int(M)
        if M < 1 or M > self.__N:
            raise ValueError('sparse: need 1 <= M <= N (M = %d, N = %d)' % (M, self.__N))
        if M == 1:
            return np.zeros(1, dtype=np.int64)
        seed = _lib.Handle(self._lib, self.__X[:1], self.__Y[:1], device=self._device)
        try:
            seed.fit(self.__hyper[:, :self.__Nx + 2])
            try:
                sel, _ = seed.append_select(self.__X[1:], None, M - 1)
            except _lib.GpmpcError as e:
                if 'single-chunk limit' in str(e):
                    raise ValueError('sparse: N - 1 = %d candidates exceed the single-chunk limit of the greedy '
                                     'selection; pass `inducing` (indices or points)' % (self.__N - 1)) from e
                raise
        finally:
            seed.close()
        if len(sel) != M - 1:
            raise ValueError('sparse: the greedy selection returned %d of %d points; pass `inducing`' % (len(sel), M - 1))
        return np.concatenate([[0], np.asarray(sel, dtype=np.int64) + 1])

    def sparse(self, M, inducing=None):
        """Fully Independent Training Conditional (FITC) model on M inducing points: what the reference names and leaves
        empty (gp_class.py:681-689, "reduce the model size from N to M").  Returns a NEW GP object whose handle is the
        sparse one (`gpmpc_sparse_fitc`): the same normalisation constants, hyper-parameters, method and bounds, X / Y
        = the inducing points Xu and the pseudo-targets Yu; every prediction costs O(M^2) instead of O(N^2).  `predict*`,
        `covar`, `discrete_linearize`, `jacobian`, `rollout*`, `validate` and `save_model` work on it (the saved file is
        the reference's format: its `load_model` predicts FITC from it); what changes data or hyper-parameters raises.
        inducing: an int array of M training indices, an (M x Nx) array of raw points (standardised here), or None =
        `sparse_default_inducing(M)`."""
        if self.__mean_func != 'zero':
            raise ValueError("sparse: FITC is built for the 'zero' mean function only")
        self._refuse_sparse('sparse')
        M = int(M)
        if M < 1 or M > self.__N:
            raise ValueError('sparse: need 1 <= M <= N (M = %d, N = %d)' % (M, self.__N))
        if inducing is None:
            Xu = self.__X[self.sparse_default_inducing(M)]
        else:
            inducing = np.asarray(inducing)
            if inducing.dtype.kind in 'iu':
                idx = inducing.reshape(-1)
                if len(idx) != M or idx.min() < 0 or idx.max() >= self.__N:
                    raise ValueError('sparse: `inducing` must hold M = %d training indices in [0, %d)' % (M, self.__N))
                Xu = self.__X[idx]
            else:
                Xu = np.array(inducing, dtype=np.float64).reshape(-1, self.__Nx)
                if Xu.shape[0] != M:
                    raise ValueError('sparse: `inducing` holds %d points, M = %d' % (Xu.shape[0], M))
                if self.__normalize:
                    Xu = self.standardize(Xu, self.__meanZ, self.__stdZ)
        Xu = np.ascontiguousarray(Xu, dtype=np.float64)
        hs = self._h.sparse_fitc(Xu, self.__hyper[:, :self.__Nx + 2])
        f = hs.get_factors(chol=True, alpha=True, invK=False)
        Yu = np.stack([f['chol'][a] @ (f['chol'][a].T @ f['alpha'][a]) for a in range(self.__Ny)], axis=1)
        g = object.__new__(GP)
        for k, v in self.__dict__.items():
            if k not in ('_h', 'train_info'):
                g.__dict__[k] = v.copy() if isinstance(v, np.ndarray) else v
        g._h = hs
        g._sparse = True
        g.__X, g.__Y, g.__N = Xu.copy(), Yu, M
        return g

    # ------------------------------------------------------------------ persistence (gp_class.py:693-743)
    def _to_dict(self, as_arrays=False):
        """Model under the key names of the reference's file format (gp_class.py:693-726), factors
        exported from the device; plain lists unless `as_arrays`."""
        f = self._h.get_factors(chol=True, alpha=True, invK=True)
        as_list = (lambda v: np.asarray(v)) if as_arrays else (lambda v: np.asarray(v).tolist())
        out = {'X': as_list(self.__X), 'Y': as_list(self.__Y),
               'hyper': {k: as_list(v) for k, v in (
                   ('hyper', self.__hyper), ('invK', f['invK']), ('alpha', f['alpha']), ('chol', f['chol']),
                   ('length_scale', self.__hyper_length_scales), ('signal_var', self.__hyper_signal_variance),
                   ('noise_var', self.__hyper_noise_variance), ('mean', self.__hyper_mean))},
               'mean_func': self.__mean_func, 'normalize': self.__normalize}
        if self.__normalize:
            for k in ('xlb', 'xub', 'ulb', 'uub'):
                out[k] = as_list(getattr(self, '_GP__' + k))
            out['meta'] = {k: as_list(getattr(self, '_GP__' + k))
                           for k in ('meanY', 'stdY', 'meanZ', 'stdZ', 'meanX', 'stdX', 'meanU', 'stdU')}
        return out

    SIDECAR_MIN_N = 1024     # from this many training points on, save_model moves the matrices out of the JSON

    def save_model(self, filename, sidecar=None):
        """Save model to `filename`.json in the reference's format (gp_class.py:729-734).

        `sidecar` (default: N >= SIDECAR_MIN_N): write the big arrays -- X, Y and hyper's chol, invK,
        alpha -- to `filename`.npz instead and leave `{"__sidecar__": key}` placeholders in the JSON
        (a JSON of Ny x N x N doubles is impractical beyond a few thousand points: 6 x 8192^2
        numbers are ~9 GB of text).  Files without a sidecar are byte-for-byte the reference's layout
        and load with the reference's GP.load_model; files with one need this class."""
        d = self._to_dict(as_arrays=True)
        if sidecar is None:
            sidecar = self.__N >= self.SIDECAR_MIN_N
        if sidecar:
            big = {'X': d['X'], 'Y': d['Y']}
            for k in ('chol', 'invK', 'alpha'):
                big['hyper_' + k] = d['hyper'][k]
                d['hyper'][k] = {'__sidecar__': 'hyper_' + k}
            d['X'] = {'__sidecar__': 'X'}
            d['Y'] = {'__sidecar__': 'Y'}
            d['sidecar_file'] = os.path.basename(filename) + '.npz'
            np.savez(filename + '.npz', **big)
        with open(filename + ".json", "w") as outfile:
            json.dump(_listify(d), outfile)

    @classmethod
    def load_model(cls, filename, **kwargs):
        """Create a new model from `filename`.json (gp_class.py:737-743); files written by the
        reference load unchanged, `__sidecar__` placeholders are resolved from the .npz next to the
        JSON.  kwargs: device=, lib=."""
        with open(filename + ".json") as json_data:
            input_dict = json.load(json_data)
        side = input_dict.pop('sidecar_file', None)
        if side is not None:
            with np.load(os.path.join(os.path.dirname(filename + '.json'), side)) as z:
                def resolve(v):
                    if isinstance(v, dict) and '__sidecar__' in v:
                        return z[v['__sidecar__']]
                    if isinstance(v, dict):
                        return {k: resolve(x) for k, x in v.items()}
                    return v
                input_dict = resolve(input_dict)
        input_dict.update(kwargs)
        return cls(**input_dict)

    # ------------------------------------------------------------------ rollout (numeric part of predict_compare)
    @staticmethod
    def lqr_gain(A, B, Q, R):
        """Infinite-horizon discrete LQR gain u = K x, the three lines of mpc_class.lqr (mpc_class.py:972-973) that
        predict_compare needs: P from the discrete algebraic Riccati equation, K = -(R + B^T P B)^-1 B^T P A."""
        import scipy.linalg
        P = np.array(scipy.linalg.solve_discrete_are(A, B, Q, R))
        return -np.array(scipy.linalg.solve(R + B.T @ P @ B, B.T @ P @ A))

    ROLLOUT_MULTI_MIN_N = 2048      # from this many training points on, rollout runs its methods in lock-step on the device

    def rollout(self, x0, u, methods=None, feedback=False, x_ref=None, Q=None, R=None, K=None, return_controls=False):
        """The numeric loop of `predict_compare` (gp_class.py:746-804) without simulator and
        plots: for every method feed (mean_t, cov_t) back into `predict` for Nt = len(u) steps.
        Returns mean[len(methods), Nt+1, Ny] and var[...] (variances un-standardised by stdY^2 and
        clipped at 0 like :795-796,826-827).

        feedback=True (gp_class.py:772-803): u_t = K (mean_t - x_ref) with the LQR gain of the model linearised at
        (x0, u[0]) (`discrete_linearize` + `lqr_gain`; pass K to use a given gain), and the control blocks of the
        input covariance K C K^T, C K^T.  DIFF: the reference subtracts x_ref (Ny,) from the (Ny x 1) array `predict`
        returns, which numpy broadcasts to an Ny x Ny matrix from the second step on ("#TODO: Fix feedback",
        gp_class.py:806); here the law is evaluated on vectors as written in its docstring."""
        Nx, Ny, Nu = self.__Nx, self.__Ny, self.__Nu
        u = np.atleast_2d(np.asarray(u, dtype=np.float64))
        Nt = u.shape[0]
        initVar = self.__hyper[:, Nx + 1] ** 2
        if methods is None:
            methods = ['EM', 'TA', 'ME']
        mean = np.zeros((len(methods), Nt + 1, Ny))
        var = np.zeros((len(methods), Nt + 1, Ny))
        controls = np.zeros((len(methods), Nt, Nu))
        covar = np.eye(Nx) * 1e-6                                               # gp_class.py:764
        # DIFF: the reference synchronises with the predictor once per step (a Python loop around GP.predict);
        # here the whole horizon runs on the device (`gpmpc_rollout`) and the result comes back once.
        for m in methods:
            if m not in METHODS:
                raise NameError('No GP method called: ' + str(m))
        x0 = np.asarray(x0, dtype=np.float64).reshape(Ny)
        norm = self.__normalize
        one = np.ones(1)
        stdX, meanX = (np.atleast_1d(self.__stdX), np.atleast_1d(self.__meanX)) if norm else (one, 0 * one)
        stdU, meanU = (np.atleast_1d(self.__stdU), np.atleast_1d(self.__meanU)) if norm else (one, 0 * one)
        stdY, meanY = (np.atleast_1d(self.__stdY), np.atleast_1d(self.__meanY)) if norm else (one, 0 * one)
        sa = stdY / stdX if norm else None                                        # x_s(next) = sa * mean_s + sb
        sb = (meanY - meanX) / stdX if norm else None
        Us = (u - meanU) / stdU
        if feedback:
            if x_ref is None:
                x_ref = np.zeros(Ny)                                              # gp_class.py:770-771
            x_ref = np.asarray(x_ref, dtype=np.float64).reshape(Ny)
            Q = np.eye(Ny) if Q is None else np.asarray(Q, dtype=np.float64)      # :765-768
            R = np.eye(Nu) if R is None else np.asarray(R, dtype=np.float64)
        keep = self.__gp_method
        if not feedback and len(methods) > 1 and self.__N >= self.ROLLOUT_MULTI_MIN_N:
            # every method from the same start, in lock-step: ONE pass over the factors per time step serves all of them
            # (gpmpc_rollout_multi; small models keep the per-method calls, whose loops are replayed from captured graphs)
            covar[:Ny, :Ny] = np.diag(initVar)
            z0 = np.concatenate([(x0 - meanX) / stdX, Us[0]])
            mean_s, cov = self._h.rollout_multi(list(methods), z0, Us, covar, sa, sb)
            for i in range(len(methods)):
                controls[i] = u
                mean[i, 0, :] = x0
                mean[i, 1:, :] = self.inverse_mean(mean_s[i], self.__meanY, self.__stdY) if norm else mean_s[i]
                var[i, 1:, :] = np.einsum('tii->ti', cov[i])
                if norm:
                    var[i, 1:, :] = self.inverse_variance(var[i, 1:, :])
            if np.any(var < 0):
                var = var.clip(min=0)
            return (mean, var, controls) if return_controls else (mean, var)
        for i, m in enumerate(methods):
            covar[:Ny, :Ny] = np.diag(initVar)                                    # gp_class.py:780 (other blocks persist)
            if feedback:
                if K is None:
                    self.set_method(m)
                    A, B = self.discrete_linearize(x0, u[0], covar)               # :785-786
                    Km = self.lqr_gain(A, B, Q, R)
                else:
                    Km = np.asarray(K, dtype=np.float64).reshape(Nu, Ny)
                u1 = Km @ (x0 - x_ref)                                            # :789-790
                z0 = np.concatenate([(x0 - meanX) / stdX, (u1 - meanU) / stdU])
                Kz = (Km * stdY[None, :]) / stdU[:, None]
                k0 = (Km @ (meanY * np.ones(Ny) - x_ref) - meanU) / stdU
                mean_s, cov, U_s = self._h.rollout_feedback(m, Nt, z0, covar, Kz, k0, Km, sa, sb)
                controls[i] = U_s * stdU + meanU
                covar[:Ny, Ny:] = cov[-1] @ Km.T                                  # what :798-803 leave behind for the
                covar[Ny:, :Ny] = covar[:Ny, Ny:].T                               # next method (covar is never reset)
                covar[Ny:, Ny:] = Km @ cov[-1] @ Km.T
            else:
                z0 = np.concatenate([(x0 - meanX) / stdX, Us[0]])
                mean_s, cov = self._h.rollout(m, z0, Us, covar, sa, sb)
                controls[i] = u
            mean[i, 0, :] = x0
            mean[i, 1:, :] = self.inverse_mean(mean_s, self.__meanY, self.__stdY) if norm else mean_s
            var[i, 1:, :] = np.einsum('tii->ti', cov)
            if norm:
                var[i, 1:, :] = self.inverse_variance(var[i, 1:, :])
        self.__gp_method = keep
        if np.any(var < 0):
            var = var.clip(min=0)
        return (mean, var, controls) if return_controls else (mean, var)

    def rollout_mc(self, x0, u, S=1000, seed=0, noise=False, feedback=False, x_ref=None, Q=None, R=None, K=None,
                   eps0=None, eps=None, return_particles=False):
        """Monte Carlo roll-out (`gpmpc_rollout_mc`): S particles drawn from the initial input distribution are propagated
        through the GP for Nt = len(u) steps on the device, every step drawing each particle's next state from the GP's
        predictive distribution at that particle's own input -- what the model itself predicts for the propagated
        distribution, where 'ME', 'TA' and 'EM' collapse it to a Gaussian at every step.  Standardisation, the initial
        covariance (eye * 1e-6 with the state block diag(sn^2)) and the gain are `rollout`'s.  Returns mean[Nt+1, Ny] and
        var[Nt+1, Ny] (row 0 = x0; sample mean and un-standardised sample variance of the particles), with
        return_particles=True also the un-standardised particles [Nt, S, Ny].

        noise=True adds the observation noise sn^2 to every draw.  feedback=True closes the loop PER PARTICLE:
        u = K (x_s - x_ref) on each particle's own state (the first control K (x0 - x_ref) is common), K the LQR gain of the
        model linearised at (x0, u[0]) unless given.  eps0[S, Nx] / eps[Nt, S, Ny] replace the generator's standard normals
        (common random numbers for comparing controllers); otherwise (seed, S) fix the result bit for bit.
        DIFF against `rollout`: after the first step the controls are exact (the 1e-6 control block of the initial covariance
        enters the initial particles only), and each step draws the outputs independently given the particle's input."""
        kw = dict(seed=seed, noise=noise, eps0=eps0, eps=eps, return_particles=return_particles)
        return self._particle_rollout(lambda Nt, z0, covar, **a: self._h.rollout_mc(S, Nt, z0, covar, **a, **kw), x0, u,
                                      feedback, x_ref, Q, R, K, return_particles)

    def _particle_rollout(self, run, x0, u, feedback, x_ref, Q, R, K, return_particles):
        """What `rollout_mc` and `rollout_paths` share: standardisation, the initial covariance, the gain, and the
        un-standardised moments (and particles) of `run(Nt, z0, covar, sa=, sb=, U= | Kz=, k0=)`."""
        Nx, Ny, Nu = self.__Nx, self.__Ny, self.__Nu
        u = np.atleast_2d(np.asarray(u, dtype=np.float64))
        Nt = u.shape[0]
        x0 = np.asarray(x0, dtype=np.float64).reshape(Ny)
        norm = self.__normalize
        one = np.ones(1)
        stdX, meanX = (np.atleast_1d(self.__stdX), np.atleast_1d(self.__meanX)) if norm else (one, 0 * one)
        stdU, meanU = (np.atleast_1d(self.__stdU), np.atleast_1d(self.__meanU)) if norm else (one, 0 * one)
        stdY, meanY = (np.atleast_1d(self.__stdY), np.atleast_1d(self.__meanY)) if norm else (one, 0 * one)
        sa = stdY / stdX if norm else None                                        # x_s(next) = sa * mean_s + sb
        sb = (meanY - meanX) / stdX if norm else None
        covar = np.eye(Nx) * 1e-6                                                 # gp_class.py:764
        covar[:Ny, :Ny] = np.diag(self.__hyper[:, Nx + 1] ** 2)                   # :780
        if feedback:
            if Nu == 0:
                raise ValueError('a closed-loop roll-out needs a model with controls')
            x_ref = np.zeros(Ny) if x_ref is None else np.asarray(x_ref, dtype=np.float64).reshape(Ny)
            if K is None:
                Q = np.eye(Ny) if Q is None else np.asarray(Q, dtype=np.float64)
                R = np.eye(Nu) if R is None else np.asarray(R, dtype=np.float64)
                A, B = self.discrete_linearize(x0, u[0], covar)
                Km = self.lqr_gain(A, B, Q, R)
            else:
                Km = np.asarray(K, dtype=np.float64).reshape(Nu, Ny)
            u1 = Km @ (x0 - x_ref)
            z0 = np.concatenate([(x0 - meanX) / stdX, (u1 - meanU) / stdU])
            Kz = (Km * stdY[None, :]) / stdU[:, None]
            k0 = (Km @ (meanY * np.ones(Ny) - x_ref) - meanU) / stdU
            res = run(Nt, z0, covar, sa=sa, sb=sb, Kz=Kz, k0=k0)
        else:
            Us = (u - meanU) / stdU
            z0 = np.concatenate([(x0 - meanX) / stdX, Us[0]]) if Nu > 0 else (x0 - meanX) / stdX
            res = run(Nt, z0, covar, sa=sa, sb=sb, U=Us if Nu > 0 else None)
        mean_s, cov = res[0], res[1]
        mean, var = np.zeros((Nt + 1, Ny)), np.zeros((Nt + 1, Ny))
        mean[0] = x0
        mean[1:] = self.inverse_mean(mean_s, self.__meanY, self.__stdY) if norm else mean_s
        v = np.einsum('tii->ti', cov)
        var[1:] = (self.inverse_variance(v) if norm else v).clip(min=0)
        if return_particles:
            return mean, var, (self.inverse_mean(res[2], self.__meanY, self.__stdY) if norm else res[2])
        return mean, var

    # ------------------------------------------------------------------ pathwise posterior samples
    def sample_paths(self, S, F=1024, seed=0):
        """Draw S functions from the posterior onto the device (`gpmpc_paths_draw`: pathwise conditioning with F random
        features of the prior, F even).  They stay valid until the data or the hyper-parameters change; `paths_eval`
        evaluates them.  F trades the prior's approximation error ("Pathwise samples") against the setup's
        N F S product."""
        self._refuse_sparse('sample_paths')
        self._h.paths_draw(S, F, seed=seed)

    def paths_eval(self, Z, grid=False):
        """The drawn paths at inputs Z in the object's units ([x, u] rows, standardised here like `predict`), outputs
        un-standardised like `predict_batch`.  grid=False: Z[S, Nx], path s at its own row, returns [S, Ny]; grid=True:
        every path at the common points Z[B, Nx], returns [S, B, Ny] (Thompson-sampling draws, plots)."""
        self._refuse_sparse('paths_eval')
        Z = np.asarray(Z, dtype=np.float64).reshape(-1, self.__Nx)
        if self.__normalize:
            Z = self.standardize(Z, self.__meanZ, self.__stdZ)
        f = self._h.paths_eval_grid(Z) if grid else self._h.paths_eval(Z)
        return self.inverse_mean(f, self.__meanY, self.__stdY) if self.__normalize else f

    def rollout_paths(self, x0, u, S=1000, F=1024, seed=0, noise=False, feedback=False, x_ref=None, Q=None, R=None, K=None,
                      eps0=None, eps=None, return_particles=False):
        """Consistent Monte Carlo roll-out (`gpmpc_rollout_paths`): `rollout_mc` with every particle propagated through ONE
        function drawn from the posterior (`sample_paths(S, F, seed)`, drawn here), so a particle that returns to a state
        sees the same dynamics there and the trajectories carry the temporal correlation the independent per-step draws
        of `rollout_mc` lose.  noise=True adds the observation noise sn eps to every step.  Arguments and return values are
        `rollout_mc`'s."""
        self._refuse_sparse('rollout_paths')
        self._h.paths_draw(S, F, seed=seed)
        kw = dict(seed=seed, noise=noise, eps0=eps0, eps=eps, return_particles=return_particles)
        return self._particle_rollout(lambda Nt, z0, covar, **a: self._h.rollout_paths(Nt, z0, covar, **a, **kw), x0, u,
                                      feedback, x_ref, Q, R, K, return_particles)

    ROLLOUT_CLOSED_LOOP_MAX = 64    # trajectories per device call (gpmpc_rollout_multi_feedback's limit)

    def rollout_closed_loop(self, X0, Nt, methods=None, x_ref=None, Q=None, R=None, K=None, u0=None, return_controls=False):
        """Closed-loop propagation (predict_compare(feedback=True), gp_class.py:772-804) of MANY trajectories in lock-step:
        for every start state in X0[S, Ny] and every method one trajectory of Nt steps under u_t = K (mean_t - x_ref),
        all of them advanced together on the device (`gpmpc_rollout_multi_feedback`: one pass over the factors per time
        step serves every 'ME' / 'TA' trajectory of a call; at most ROLLOUT_CLOSED_LOOP_MAX trajectories per call, more
        are split over several calls).  The gain is the LQR gain of the model linearised at (start, u0) -- `u0` defaults
        to zeros -- by `discrete_linearize` + `lqr_gain` under that trajectory's method, unless `K` ([Nu, Ny], or
        [S, Nu, Ny]: one per start) is given.  Returns mean[S, len(methods), Nt+1, Ny] and var[...] (un-standardised and
        clipped at 0 like `rollout`), with return_controls=True also the controls applied [S, len(methods), Nt, Nu].

        DIFF: every trajectory starts from the reference's FRESH initial input covariance (eye(Nx) * 1e-6 with the state
        block diag(sn^2), gp_class.py:764,780).  The reference's loop -- and `rollout(feedback=True)`, which follows it
        literally -- never resets `covar` between methods: the control blocks method i leaves after its last step are
        part of method i+1's initial covariance (gp_class.py:777-804), so its methods are not independent trajectories
        and cannot advance in lock-step.  A single-method `rollout(feedback=True)` is the same trajectory as here."""
        Nx, Ny, Nu = self.__Nx, self.__Ny, self.__Nu
        if Nu == 0:
            raise ValueError('a closed-loop roll-out needs a model with controls')
        X0 = np.atleast_2d(np.asarray(X0, dtype=np.float64)).reshape(-1, Ny)
        S, Nt = X0.shape[0], int(Nt)
        if methods is None:
            methods = ['EM', 'TA', 'ME']
        for m in methods:
            if m not in METHODS:
                raise NameError('No GP method called: ' + str(m))
        nm = len(methods)
        norm = self.__normalize
        one = np.ones(1)
        stdX, meanX = (np.atleast_1d(self.__stdX), np.atleast_1d(self.__meanX)) if norm else (one, 0 * one)
        stdU, meanU = (np.atleast_1d(self.__stdU), np.atleast_1d(self.__meanU)) if norm else (one, 0 * one)
        stdY, meanY = (np.atleast_1d(self.__stdY), np.atleast_1d(self.__meanY)) if norm else (one, 0 * one)
        sa = stdY / stdX if norm else None                                        # x_s(next) = sa * mean_s + sb
        sb = (meanY - meanX) / stdX if norm else None
        x_ref = np.zeros(Ny) if x_ref is None else np.asarray(x_ref, dtype=np.float64).reshape(Ny)   # gp_class.py:770-771
        Q = np.eye(Ny) if Q is None else np.asarray(Q, dtype=np.float64)          # :765-768
        R = np.eye(Nu) if R is None else np.asarray(R, dtype=np.float64)
        u0 = np.zeros(Nu) if u0 is None else np.asarray(u0, dtype=np.float64).reshape(Nu)
        if K is not None:
            K = np.broadcast_to(np.asarray(K, dtype=np.float64).reshape(-1, Nu, Ny), (S, Nu, Ny))
        covar = np.eye(Nx) * 1e-6                                                 # gp_class.py:764
        covar[:Ny, :Ny] = np.diag(self.__hyper[:, Nx + 1] ** 2)                   # :780
        Z0, Kz, k0, Kc = (np.zeros((S, nm, Nx)), np.zeros((S, nm, Nu, Ny)), np.zeros((S, nm, Nu)), np.zeros((S, nm, Nu, Ny)))
        keep = self.__gp_method
        for s in range(S):
            gains = {}
            for i, m in enumerate(methods):
                if K is not None:
                    Km = K[s]
                else:
                    kind = 'EM' if m == 'EM' else 'mean'         # (only 'EM' linearises another mean: discrete_linearize)
                    if kind not in gains:
                        self.set_method(m)
                        A, B = self.discrete_linearize(X0[s], u0, covar)          # :785-786
                        gains[kind] = self.lqr_gain(A, B, Q, R)
                    Km = gains[kind]
                u1 = Km @ (X0[s] - x_ref)                                         # :789-790
                Z0[s, i] = np.concatenate([(X0[s] - meanX) / stdX, (u1 - meanU) / stdU])
                Kz[s, i] = (Km * stdY[None, :]) / stdU[:, None]
                k0[s, i] = (Km @ (meanY * np.ones(Ny) - x_ref) - meanU) / stdU
                Kc[s, i] = Km
        self.__gp_method = keep
        flat = lambda a: a.reshape((S * nm,) + a.shape[2:])
        Z0, Kz, k0, Kc = flat(Z0), flat(Kz), flat(k0), flat(Kc)
        codes = list(methods) * S
        mean_s, cov, U_s = np.zeros((S * nm, Nt, Ny)), np.zeros((S * nm, Nt, Ny, Ny)), np.zeros((S * nm, Nt, Nu))
        for lo in range(0, S * nm, self.ROLLOUT_CLOSED_LOOP_MAX):
            hi = min(lo + self.ROLLOUT_CLOSED_LOOP_MAX, S * nm)
            mean_s[lo:hi], cov[lo:hi], U_s[lo:hi] = self._h.rollout_multi_feedback(
                codes[lo:hi], Z0[lo:hi], covar, Kz[lo:hi], k0[lo:hi], Kc[lo:hi], sa=sa, sb=sb, T=Nt)
        mean = np.zeros((S, nm, Nt + 1, Ny))
        var = np.zeros((S, nm, Nt + 1, Ny))
        mean[:, :, 0, :] = X0[:, None, :]
        mean[:, :, 1:, :] = (self.inverse_mean(mean_s, self.__meanY, self.__stdY) if norm else mean_s).reshape(S, nm, Nt, Ny)
        v = np.einsum('ktii->kti', cov)
        var[:, :, 1:, :] = (self.inverse_variance(v) if norm else v).reshape(S, nm, Nt, Ny)
        if np.any(var < 0):
            var = var.clip(min=0)
        controls = (U_s * stdU + meanU).reshape(S, nm, Nt, Nu)
        return (mean, var, controls) if return_controls else (mean, var)

    def predict_compare(self, x0, u, model=None, num_cols=2, xnames=None, title=None, feedback=False, x_ref=None,
                        Q=None, R=None, methods=None, mc=None, mc_paths=None):
        """`predict_compare` (gp_class.py:746-861) without its matplotlib front end: the T-step uncertainty propagation
        of every method in `methods` (default ['EM', 'TA', 'ME'], :759-760) through `GP.rollout` -- the whole horizon on
        the device -- next to the simulated trajectory of `model` when one is given (`model.sim(x0, u)`, :819-820;
        model_class needs casadi + SUNDIALS and is out of scope, so any object with that method -- and
        `sampling_time()` for the time axis, :756 -- does).  The scripts that call it (van_der_pol.py:83-85,
        tank_example.py) keep running; instead of figures they get the arrays the figures were drawn from:

            {'t': [Nt+1], 'methods': [...], 'mean': [M, Nt+1, Ny], 'var': [M, Nt+1, Ny] (clipped at 0, :826-827),
             'y_sim': [Nt+1, Ny] or None}

        num_cols, xnames, title only shaped the plot and are accepted for signature compatibility.
        mc=S adds 'mc_mean' and 'mc_var' [Nt+1, Ny]: the Monte Carlo roll-out of S particles (`rollout_mc`, seed 0) under the
        same controls or feedback arguments -- the model's own predictive distribution, against which the methods'
        approximations can be judged.  Without it the dict is the one above, key for key.  mc_paths=F (with mc=S) takes the
        consistent roll-out instead (`rollout_paths`: S functions of F features drawn once)."""
        u = np.atleast_2d(np.asarray(u, dtype=np.float64))
        Nt = u.shape[0]
        if methods is None:
            methods = ['EM', 'TA', 'ME']
        mean, var = self.rollout(x0, u, methods=methods, feedback=feedback, x_ref=x_ref, Q=Q, R=R)
        y_sim, dt = None, 1.0
        if model is not None:
            if hasattr(model, 'sampling_time'):
                dt = float(model.sampling_time())
            if hasattr(model, 'sim'):
                y_sim = np.vstack([np.asarray(x0, dtype=np.float64).reshape(1, -1),
                                   np.asarray(model.sim(x0, u), dtype=np.float64).reshape(Nt, -1)])   # :819-820
        out = {'t': np.linspace(0.0, Nt * dt, Nt + 1), 'methods': list(methods), 'mean': mean, 'var': var.clip(min=0),
               'y_sim': y_sim}
        if mc is not None:
            if mc_paths is None:
                out['mc_mean'], out['mc_var'] = self.rollout_mc(x0, u, S=int(mc), feedback=feedback, x_ref=x_ref, Q=Q, R=R)
            else:
                out['mc_mean'], out['mc_var'] = self.rollout_paths(x0, u, S=int(mc), F=int(mc_paths), feedback=feedback,
                                                                   x_ref=x_ref, Q=Q, R=R)
        return out

    def close(self):
        if self._h is not None:
            self._h.close()
            self._h = None
