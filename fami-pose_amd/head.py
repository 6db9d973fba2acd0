"""What supervises the final heat map of a training step: targets, loss terms and seeds, between the forward and the backward
pass (train.Trainer owns one SupervisionHead and calls it from _forward_backward)."""
from types import SimpleNamespace

import torch

from .engine import _p


class ScalarTerm:
    """A loss term kept beside `loss_parts` (which keeps its 7 entries): a one-element device scalar of the last step, under
    accumulation {open window, last closed window} sums of it, the 'grad_accum' checkpoint key of the open window's sum and
    what a checkpoint that lacks the key was written without."""

    def __init__(self, name, key, without, dev, window):
        self.name, self.key, self.without = name, key, without
        self.value = torch.zeros(1, device=dev)
        self.window = torch.zeros(2, 1, device=dev) if window else None


class SupervisionHead:
    """The options are fixed at construction and baked into the captured plans; the defaults leave the three launches
    fami_gauss_target_f32 / fami_wmse_fwd_f32 / fami_wmse_bwd_f32 (train.Trainer's docstring says what each option computes).

    targets(): fami_gauss_target_f32, or with joint_weights / target_encoding='subpixel' fami_gauss_target_ex_f32.
    forward(), in this order:
    * fami_wmse_fwd_f32, or with ohkm_topk fami_ohkm_fwd_f32 in its place: it ranks the J row losses of each sample on the
      device and writes the selected weights, which the heat-map seed then reads;
    * with either coordinate term fami_softargmax_fwd_f32 (at softargmax_beta) and fami_heatmap_xy_f32, both ONCE, their buffers
      shared; then fami_integral_l1_fwd_f32 (integral_l1_weight) and fami_structure_cos_fwd_f32 (structure_cos_weight).  Both
      read the target weights, also where OHKM selects, and write a ScalarTerm of `terms` (integral first);
    * with pck the two fami_pck_accuracy_f32 rows of `acc` (final and key-frame maps against the target map).
    The seed() it returns, all under the host or the device loss scale: fami_wmse_bwd_f32 writes the seed buffer;
    fami_integral_l1_bwd_f32 adds to it (accumulate = 1); fami_structure_cos_bwd_f32 then fami_softargmax_bwd_f32 (accumulate = 1);
    Engine.seed_nchw; with use_mi the six MI values into loss_parts[1:7] and their seeds on three lanes, accumulated in term
    order on lane 0.

    Per batch shape (B, J) one record of `bufs` holds what the launches write and a later call reads -- the accessors, the
    seeds, a replayed plan: sel_w [B*J] (OHKM's selected weights), coords / stats / txy [B*J,2] (soft-argmax and target
    positions), gcoords [B*J,2] and tw [B*J] (the structure term's coordinate gradient and the target weights
    structure_cosines() reads).  A record is made once and never replaced -- captured plans hold its addresses -- and holds
    only what this configuration launches into (None otherwise; no record at all without such an option).  `shape` is the
    (B, J) of the last step: Trainer.step sets it, since a graph replay does not pass through here."""

    def __init__(self, model, targets_from_joints, sigma, mse_weight, alpha, beta, use_mi, pck, target_encoding, joint_weights,
                 ohkm_topk, integral_l1_weight, integral_beta, structure_cos_weight, structure_pairs, structure_min_len):
        """validates the options (host arithmetic only; place() makes the device state)"""
        from .loss import check_integral_options, check_ohkm_topk, check_structure_options, check_target_options
        self.integral_l1_weight = self.softargmax_beta = None
        if integral_l1_weight is not None:
            self.integral_l1_weight, self.softargmax_beta = check_integral_options(integral_l1_weight, integral_beta)
            if not targets_from_joints:
                raise ValueError('integral_l1_weight supervises the joint position itself: it needs targets_from_joints=True '
                                 '(precomputed targets carry no real-valued position; loss.IntegralL1Loss takes one)')
        num_joints = getattr(model, 'num_joints', None)
        self.structure_cos_weight = self.structure_pairs = self.structure_min_len = self.structure_eps = None
        if structure_cos_weight is not None:
            from .data import LIMB_PAIRS
            _, self.softargmax_beta = check_integral_options(1.0, integral_beta)
            self.structure_cos_weight, self.structure_pairs, self.structure_min_len, self.structure_eps = check_structure_options(
                structure_cos_weight, LIMB_PAIRS if structure_pairs is None else structure_pairs, structure_min_len, 1e-8, num_joints)
            if not targets_from_joints:
                raise ValueError('structure_cos_weight supervises the joint position itself: it needs targets_from_joints=True '
                                 '(precomputed targets carry no real-valued position; loss.StructureCosineSimilarity takes one)')
        self.subpixel, self.joint_weights = check_target_options(target_encoding, joint_weights, num_joints)
        if (self.subpixel or self.joint_weights is not None) and not targets_from_joints:
            raise ValueError("target_encoding='subpixel' and joint_weights act where the Trainer makes the targets: they need "
                             "targets_from_joints=True (precomputed targets: loss.generate_heatmaps takes both)")
        self.ohkm_topk = None if ohkm_topk is None else check_ohkm_topk(ohkm_topk, num_joints)
        self.targets_from_joints, self.sigma, self.pck = targets_from_joints, sigma, pck
        self.mse_weight, self.alpha, self.beta, self.use_mi = mse_weight, alpha, beta, use_mi

    def place(self, dev, windows):
        """the device state; windows: gradient accumulation is on, every scalar term keeps a window sum"""
        self.dev = dev
        self.loss_parts = torch.zeros(7, device=dev)     # mse, mi_1..6 (device scalars of the last step)
        self.acc = None           # [2, J+3] device floats of the last step: PCK of final_hm / kf_bb_hm (Trainer.accuracy)
        self.joint_w = None if self.joint_weights is None else torch.tensor(self.joint_weights, dtype=torch.float32, device=dev)
        self.bufs, self.shape = {}, None
        self.integral = (None if self.integral_l1_weight is None else
                         ScalarTerm('integral', 'integral_loss_sum', 'the integral L1 term', dev, windows))
        self.structure = (None if self.structure_cos_weight is None else
                          ScalarTerm('structure', 'structure_loss_sum', 'the structure cosine term', dev, windows))
        self.pairs_dev = (None if self.structure is None else
                          torch.tensor(self.structure_pairs, dtype=torch.int32).reshape(-1, 2).to(dev))
        self.integral_loss, self.structure_loss = (None if t is None else t.value for t in (self.integral, self.structure))
        self.terms = [t for t in (self.integral, self.structure) if t is not None]

    def _record(self, B, J):
        """the (B, J) record of `bufs` (class docstring); None where this configuration keeps nothing per shape"""
        if self.ohkm_topk is None and self.softargmax_beta is None:
            return None
        if (B, J) not in self.bufs:
            zeros = lambda on, *shape: torch.zeros(*shape, device=self.dev) if on else None  # noqa: E731
            coords, structure = self.softargmax_beta is not None, self.structure is not None
            self.bufs[(B, J)] = SimpleNamespace(
                sel_w=zeros(self.ohkm_topk is not None, B * J), coords=zeros(coords, B * J, 2), stats=zeros(coords, B * J, 2),
                txy=zeros(coords, B * J, 2), gcoords=zeros(structure, B * J, 2), tw=zeros(structure, B * J))
        return self.bufs[(B, J)]

    def targets(self, eng, kf_x, target, weight):
        """-> (target map, target weights, joints).  targets_from_joints: `target` carries joints [B,J,2] and `weight` the
        visibility [B,J]; the Gaussian maps are made on the device (generate_heatmaps)."""
        if not self.targets_from_joints:
            return target, weight, None
        joints, vis = target, weight
        B, J = joints.shape[:2]
        Hh, Wh = kf_x.shape[2] // 4, kf_x.shape[3] // 4
        target = eng.empty(B, J, Hh, Wh)
        # structure_cosines() reads the step's target weights afterwards: then a buffer of the head's own
        weight = eng.empty(B, J) if self.structure is None else self._record(B, J).tw.view(B, J)
        if self.subpixel or self.joint_w is not None:
            if self.joint_w is not None and self.joint_w.numel() != J:
                raise ValueError('joint_weights holds %d values, the batch has %d joints' % (self.joint_w.numel(), J))
            eng.call('fami_gauss_target_ex_f32', _p(joints), _p(vis), _p(self.joint_w), _p(target), _p(weight), B, J,
                     Hh, Wh, kf_x.shape[2], kf_x.shape[3], self.sigma, int(self.subpixel))
        else:
            eng.call('fami_gauss_target_f32', _p(joints), _p(vis), _p(target), _p(weight), B, J, Hh, Wh,
                     kf_x.shape[2], kf_x.shape[3], self.sigma)
        return target, weight, joints

    def forward(self, eng, kf_x, outs, target, weight, joints):
        """the loss terms and the PCK rows of the step -> seed(ls, ls_dev): it enqueues the seeds of the backward pass under the
        loss scale (a host factor, or 1 and the device scalar the scale update rewrites) and returns the seed buffer -- not an
        Engine buffer: the caller holds it until the backward pass is enqueued"""
        final, aux = outs[0], eng.aux
        B, J, Hh, Wh = final.shape
        L, r = Hh * Wh, self._record(B, J)
        scale = self.mse_weight / (B * L * (J if self.ohkm_topk is None else self.ohkm_topk))
        w = tw = weight.reshape(B * J)
        ws = eng.ws(B * J * 4)
        if self.ohkm_topk is None:
            eng.call('fami_wmse_fwd_f32', _p(final), _p(target), _p(w), _p(self.loss_parts[0:1]), B * J, L, float(scale), _p(ws))
        else:
            # the selection between the loss rows and the seeds, on the device: the heat-map seed reads the selected weights
            if self.ohkm_topk > J:
                raise ValueError('ohkm_topk = %d, the model has %d joints' % (self.ohkm_topk, J))
            eng.call('fami_ohkm_fwd_f32', _p(final), _p(target), _p(w), _p(self.loss_parts[0:1]), _p(r.sel_w), B, J, L,
                     self.ohkm_topk, float(scale), _p(ws))
            w = r.sel_w
        if self.softargmax_beta is not None:
            # the coordinate terms: soft-argmax of the final map against joint / stride, on the TARGET weights `tw` (not OHKM's);
            # coordinates and target positions once, whichever of the two terms read them
            eng.call('fami_softargmax_fwd_f32', _p(final), _p(r.coords), _p(r.stats), B * J, Hh, Wh, self.softargmax_beta)
            eng.call('fami_heatmap_xy_f32', _p(joints), _p(r.txy), B * J, Hh, Wh, kf_x.shape[2], kf_x.shape[3])
        if self.integral is not None:
            iscale = self.integral_l1_weight / (B * J)
            eng.call('fami_integral_l1_fwd_f32', _p(r.coords), _p(r.txy), _p(tw), _p(self.integral.value), B * J, Hh, Wh,
                     float(iscale), _p(eng.ws(B * J * 4)))
        if self.structure is not None:
            P = len(self.structure_pairs)
            sscale = self.structure_cos_weight / (B * P)
            eng.call('fami_structure_cos_fwd_f32', _p(r.coords), _p(r.txy), _p(tw), _p(self.pairs_dev), _p(self.structure.value),
                     B, J, P, self.structure_min_len, self.structure_eps, float(sscale), _p(eng.ws(B * P * 4)))
        if self.pck:
            # accuracy(pred_heatmaps, target) and accuracy(kf_bb_heatmaps, target), core fn :159-163, without the four
            # device-to-host heatmap copies
            if self.acc is None or self.acc.shape[1] != J + 3:
                self.acc = torch.zeros(2, J + 3, device=self.dev)
            iws = eng.empty(2 * B * J, dtype=torch.int64)
            mws = eng.empty(2 * B * J)
            for k, hm in enumerate((final, outs[1])):
                eng.call('fami_pck_accuracy_f32', _p(hm), _p(target), _p(self.acc[k]), _p(iws), _p(mws), B, J, Hh, Wh, 0.5)

        def seed(ls, ls_dev):
            dpred = torch.empty_like(final)
            eng.call('fami_wmse_bwd_f32', _p(final), _p(target), _p(w), _p(dpred), B * J, L, float(scale * ls), _p(ls_dev), 0)
            if self.integral is not None:
                eng.call('fami_integral_l1_bwd_f32', _p(final), _p(r.coords), _p(r.stats), _p(r.txy), _p(tw), _p(dpred), B * J,
                         Hh, Wh, self.softargmax_beta, float(iscale * ls), _p(ls_dev), 1)
            if self.structure is not None:
                eng.call('fami_structure_cos_bwd_f32', _p(r.coords), _p(r.txy), _p(tw), _p(self.pairs_dev), _p(r.gcoords), B, J, P,
                         self.structure_min_len, self.structure_eps, float(sscale * ls), _p(ls_dev))
                eng.call('fami_softargmax_bwd_f32', _p(final), _p(r.coords), _p(r.stats), _p(r.gcoords), _p(dpred), B * J, Hh, Wh,
                         self.softargmax_beta, 1)
            eng.seed_nchw(aux['final'], dpred)
            if self.use_mi and aux['mis']:
                self._seed_mi(eng, aux, ls, ls_dev)
            return dpred
        return seed

    def _seed_mi(self, eng, aux, ls, ls_dev):
        """the six MI values into loss_parts[1:7] and their seeds"""
        a, b = self.alpha, self.beta
        coef = [-b * a, b * a, a, -a, a, -a]        # core fn :119-148
        if eng.use_lanes:      # the six seeds on three lanes
            eng._do_fork(3)        # (not taped: the seeds are enqueued here, ahead of the tape walk)
        pending = []
        same = aux.get('mi_same', {})      # repeated terms (mi_6 is mi_2): one gradient pass with the summed coefficient
        for k, j in same.items():
            coef[j] += coef[k]
        for k, ((val, seed), c) in enumerate(zip(aux['mis'], coef)):
            if eng.use_lanes:
                eng.set_lane(k % 3)
            eng.call('fami_axpby_f32', _p(val), None, _p(self.loss_parts[1 + k:2 + k]), 1, 1.0, 0.0)
            if k not in same:
                pending.append(seed(c * ls, ls_dev, True))
        if eng.use_lanes:
            eng._do_join(3)
        for fin in pending:        # the accumulations into the (shared) gradient buffers, in term order, on lane 0
            fin()

    def _last(self, field):
        """`field` of the last step's record (None before the first step, or where the configuration keeps none)"""
        return getattr(self.bufs.get(self.shape), field, None)

    def ohkm_selection(self):
        sel = self._last('sel_w')
        return None if sel is None else (sel != 0).reshape(self.shape)

    def integral_coords(self):
        coords = self._last('coords')
        return None if coords is None else coords.reshape(*self.shape, 2)

    def structure_cosines(self):
        if self._last('tw') is None:
            return None
        from .loss import limb_cosines
        (B, J), r = self.shape, self.bufs[self.shape]
        return limb_cosines(r.coords.reshape(B, J, 2), r.txy.reshape(B, J, 2), r.tw.reshape(B, J), self.structure_pairs,
                            self.structure_min_len, self.structure_eps)
