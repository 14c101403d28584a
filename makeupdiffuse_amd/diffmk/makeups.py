"""``diffmk.makeups`` — the inference-side surface of the reference's DDIM-inversion fine-tune model
(reference diffmk/makeups.py), i.e. the only callers of ``MKDDIMSampler.reconstruct`` in the reference:

  * ``on_fit_start``        :44-47   builds the sampler, ``make_schedule(ddim_num_steps=iter_finetune)``
  * ``generate_image``      :119-127 ``reconstruct(x_latent=inv, cond=c, t_start=iter_finetune)`` -> ``decode_latent_code``
                                     -> ``(x + 1) / 2`` clamped to [0, 1]
  * ``decode_latent_code``  :260-262 ``first_stage_model.decode(z / scale_factor)``
  * ``log_images``          :265-286 the two reconstructions (source under the reference hint, reference under the source hint)

The losses (:80-245) as TRAINING code are out of scope: ``shared_step`` / ``p_losses`` / ``forward`` raise.  Their
evaluation use (the reference runs them under ``prefix = 'val'`` too) is here without gradients: ``validation_losses`` and the
``p_loss_*`` / ``criterionHis`` / ``get_msk_*`` methods, the histogram terms on the device through ``makeup_score``.
The hint of this variant is ONE image (``c_concat_r`` / ``c_concat_s``, 3 channels): build the model from a
``control_stage_config`` with ``hint_channels: 3``.  The arithmetic runs in libmkd; nothing here has a CPU path."""
from __future__ import annotations

from typing import Dict, Optional

import torch

from .. import makeup_score as _ms
from .cddim import MKDDIMSampler
from .makeup_diffuse import BaseMakeUpDiffuse


class BaseModel(BaseMakeUpDiffuse):
    def __init__(self, src_msk_key: str = 'src_msk', ref_msk_key: str = 'ref_msk', src_img_key: str = 'src_img',
                 src_inv_key: str = 'src_inv', ref_img_key: str = 'ref_img', ref_inv_key: str = 'ref_inv', dataset_len: int = 0,
                 t0: int = 1000, inv_steps: int = 50, iter_finetune: int = 50, debug_dir: Optional[str] = None,
                 weight_loss_cycle: float = 0.0, weight_loss_makeup: float = 1.0, weight_loss_idt: float = 0.0,
                 weight_loss_background: float = 1.0, lambda_his_lip: float = 1.0, lambda_his_skin_1: float = 1.0,
                 lambda_his_skin_2: float = 1.0, lambda_his_eye: float = 1.0, loss_type: str = 'l1', *args, **kwargs):
        super().__init__(*args, src_img_key=src_img_key, ref_img_key=ref_img_key, **kwargs)
        self.weight_loss_cycle, self.weight_loss_makeup = weight_loss_cycle, weight_loss_makeup
        self.weight_loss_idt, self.weight_loss_background = weight_loss_idt, weight_loss_background
        self.lambda_his_lip, self.lambda_his_eye = lambda_his_lip, lambda_his_eye
        self.lambda_his_skin_1, self.lambda_his_skin_2 = lambda_his_skin_1, lambda_his_skin_2
        self.loss_type = loss_type
        self.src_inv_key, self.ref_inv_key = src_inv_key, ref_inv_key
        self.src_msk_key, self.ref_msk_key = src_msk_key, ref_msk_key
        self.dataset_len, self.debug_dir = dataset_len, debug_dir
        self.t0, self.inv_steps, self.iter_finetune = t0, inv_steps, iter_finetune
        self.ddim_sampler: Optional[MKDDIMSampler] = None

    def update_schedule(self) -> None:
        """:40-42: re-registers the LINEAR beta schedule with ``timesteps = t0`` (same linear_start / linear_end): the DDIM
        inversion and its fine-tune run on a t0-step DDPM chain."""
        self.register_schedule(given_betas=None, beta_schedule='linear', timesteps=self.t0, linear_start=self.linear_start,
                               linear_end=self.linear_end, cosine_s=8e-3)

    def on_fit_start(self) -> None:
        """:44-47."""
        self.update_schedule()
        self.ddim_sampler = MKDDIMSampler(self)
        self.ddim_sampler.make_schedule(ddim_num_steps=self.iter_finetune)

    def _sampler(self) -> MKDDIMSampler:
        if self.ddim_sampler is None:
            self.on_fit_start()
        return self.ddim_sampler

    @torch.no_grad()
    def get_input(self, batch: dict, k, bs: Optional[int] = None, *args, **kwargs):
        """:70-78 -> (src_inv, ref_inv, src_msk, ref_msk, c) with c_concat_s = [src_img], c_concat_r = [ref_img]."""
        src = self.get_origin_img_input(batch, self.src_img_key, bs)
        ref = self.get_origin_img_input(batch, self.ref_img_key, bs)
        msk = lambda key: batch[key].to(self.device) if key in batch else None
        c = dict(c_crossattn=[self.get_cond_txt_coding(batch, bs)], c_concat_s=[src], c_concat_r=[ref])
        return batch[self.src_inv_key].to(self.device), batch[self.ref_inv_key].to(self.device), msk(self.src_msk_key), msk(self.ref_msk_key), c

    @torch.no_grad()
    def generate_image(self, inv: torch.Tensor, c: dict, c_replace=None, c_type: str = 'c_concat_r') -> torch.Tensor:
        """:119-127.  Mutates ``c['c_concat']`` exactly as the reference does."""
        c['c_concat'] = c_replace if c_replace else c[c_type]
        z = self._sampler().reconstruct(x_latent=inv, cond=c, t_start=self.iter_finetune)
        img = (self.decode_latent_code(z) + 1.0) / 2.0
        return img.clamp(0, 1)

    @torch.no_grad()
    def invert_image(self, img: torch.Tensor, c: dict, t_enc: Optional[int] = None, seeds=None) -> torch.Tensor:
        """The inversion that produces ``src_inv`` / ``ref_inv`` (reference pre_dataset.py InvRec): z = get_z(img * 2 - 1), then
        the DDIM inversion ``encode(z, c, t_enc)`` under c_crossattn with c_concat = None (the UNet alone).  img [B,3,H,W] in
        [0, 1]; t_enc defaults to iter_finetune, the step count generate_image reconstructs with.  Needs first_stage_encoder=True.  ``seeds``
        (get_z's): the posterior sample comes from noise.normal on stream 3, the inversion itself is deterministic."""
        z = self.get_z(img * 2.0 - 1.0, **({} if seeds is None else {'seeds': seeds}))
        cond = dict(c_crossattn=list(c['c_crossattn']), c_concat=None)
        inv, _ = self._sampler().encode(z, cond, self.iter_finetune if t_enc is None else int(t_enc))
        return inv

    @torch.no_grad()
    def log_images(self, batch: dict, **kwargs) -> Dict[str, torch.Tensor]:
        """:265-286: source latent re-generated under the reference hint and vice versa."""
        src_inv, ref_inv, _, _, c = self.get_input(batch, self.first_stage_key)
        log: Dict[str, torch.Tensor] = {}
        c['c_concat'] = c['c_concat_r']
        log['rec_src_ref'] = self.decode_first_stage(self._sampler().reconstruct(x_latent=src_inv, cond=c, t_start=self.iter_finetune))
        c['c_concat'] = c['c_concat_s']
        log['rec_ref_src'] = self.decode_first_stage(self._sampler().reconstruct(x_latent=ref_inv, cond=c, t_start=self.iter_finetune))
        log['ori_src'] = torch.cat(c['c_concat_s'], 0) * 2.0 - 1.0
        log['ori_ref'] = torch.cat(c['c_concat_r'], 0) * 2.0 - 1.0
        return log

    # ---- evaluation losses (:90-245 under prefix 'val'), no gradients -----------------------------------------------------
    # Label maps are [B,H,W] / [B,1,H,W] / [B,H,W,1]; every pair of a batch is scored on its own (the reference assumes batch 1)
    # and a loss is the mean over the pairs.  Where the reference returns index lists, these return the pixel counts [B].
    def get_loss(self, pred: torch.Tensor, target: torch.Tensor, mean: bool = True) -> torch.Tensor:
        """UPSTREAM DDPM.get_loss."""
        if self.loss_type == 'l1':
            loss = (target - pred).abs()
        elif self.loss_type == 'l2':
            loss = (target - pred) ** 2
        else:
            raise NotImplementedError(f"unknown loss type '{self.loss_type}'")
        return loss.mean() if mean else loss

    def get_msk_lip(self, mask_A, mask_B):
        """:179-183 -> (mask_A_lip, mask_B_lip, count_A, count_B), masks uint8 [B,H,W]."""
        (a, ca, _), (b, cb, _) = _ms.region_mask(mask_A, _ms.LIP_CLASSES), _ms.region_mask(mask_B, _ms.LIP_CLASSES)
        return a, b, ca, cb

    def get_msk_skin(self, mask_A, mask_B):
        """:185-189."""
        (a, ca, _), (b, cb, _) = _ms.region_mask(mask_A, _ms.SKIN_CLASSES), _ms.region_mask(mask_B, _ms.SKIN_CLASSES)
        return a, b, ca, cb

    def get_msk_eye(self, mask_A, mask_B):
        """:191-204 -> (A_left, B_left, count_A_left, count_B_left, A_right, B_right, count_A_right, count_B_right)."""
        out = []
        for eye in (_ms.EYE_LEFT_CLASSES, _ms.EYE_RIGHT_CLASSES):
            (a, ca, _), (b, cb, _) = (_ms.region_mask(m, _ms.FACE_CLASSES, eye, _ms.EYE_MARGIN) for m in (mask_A, mask_B))
            out += [a, b, ca, cb]
        return tuple(out)

    @torch.no_grad()
    def criterionHis(self, input_data, target_data, mask_src, mask_tar, index=None) -> torch.Tensor:
        """:232-245 -> [B]: L1 between input * 255 under mask_src and its histogram match to target under mask_tar
        (``index`` is the reference's pixel list; the masks carry the same information and it is ignored)."""
        return _ms.histogram_match(input_data, target_data, mask_src, mask_tar, want_matched=False)[2]

    def _hist_terms(self, SR, RS, src_msk, ref_msk, S, R) -> Dict[str, torch.Tensor]:
        return _ms.makeup_hist_terms(SR, RS, S, R, src_msk, ref_msk, lambdas=dict(
            lip=self.lambda_his_lip, skin_1=self.lambda_his_skin_1, skin_2=self.lambda_his_skin_2, eye=self.lambda_his_eye))

    @torch.no_grad()
    def p_loss_hist_lip(self, SR, RS, src_msk, ref_msk, S, R):
        """:159-163 -> (sr_lip, rs_lip), [B] each."""
        t = self._hist_terms(SR, RS, src_msk, ref_msk, S, R)
        return t['sr_lip'], t['rs_lip']

    @torch.no_grad()
    def p_loss_hist_skin(self, SR, RS, src_msk, ref_msk, S, R):
        """:165-169."""
        t = self._hist_terms(SR, RS, src_msk, ref_msk, S, R)
        return t['sr_skin'], t['rs_skin']

    @torch.no_grad()
    def p_loss_hist_eye(self, SR, RS, src_msk, ref_msk, S, R):
        """:171-177 -> (sr_left, rs_left, sr_right, rs_right)."""
        t = self._hist_terms(SR, RS, src_msk, ref_msk, S, R)
        return t['sr_eye_left'], t['rs_eye_left'], t['sr_eye_right'], t['rs_eye_right']

    @torch.no_grad()
    def p_loss_makeup(self, SR, RS, src_msk, ref_msk, S, R, return_terms: bool = False):
        """:147-153, literally: the skin bracket is sr_skin + sr_skin.  Mean over the pairs; return_terms: also the dict of the
        eight per-pair terms (makeup_score.makeup_hist_terms), so that nobody has to rely on that expression."""
        t = self._hist_terms(SR, RS, src_msk, ref_msk, S, R)
        return (t['loss_makeup'].mean(), t) if return_terms else t['loss_makeup'].mean()

    @torch.no_grad()
    def p_loss_background(self, SR, RS, src_msk, ref_msk, S, R) -> torch.Tensor:
        """:129-140: background 0, hair 10, neck 13."""
        def sel(m):
            lab = _ms.label_map(m).to(SR.device)[:, None]
            return (lab == 0) | (lab == 10) | (lab == 13)
        loss_s = (self.get_loss(SR, S, mean=False) * sel(src_msk)).mean([1, 2, 3])
        loss_r = (self.get_loss(RS, R, mean=False) * sel(ref_msk)).mean([1, 2, 3])
        return (loss_s.mean() + loss_r.mean()) * 0.5

    @torch.no_grad()
    def p_loss_idt(self, SS, RR, S, R) -> torch.Tensor:
        """:142-145."""
        loss_s = self.get_loss(SS, S, mean=False).mean([1, 2, 3])
        loss_r = self.get_loss(RR, R, mean=False).mean([1, 2, 3])
        return (loss_s.mean() + loss_r.mean()) * 0.5

    @torch.no_grad()
    def p_loss_cycle(self, r_S, r_R, S, R) -> torch.Tensor:
        """:155-156."""
        return self.p_loss_idt(SS=r_S, RR=r_R, S=S, R=R)

    @torch.no_grad()
    def validation_losses(self, batch: dict, return_images: bool = False):
        """What the reference's ``p_losses`` computes under ``prefix = 'val'`` (:90-117) -> (loss, loss_dict): the same
        generate_image calls, weights and 'val/...' keys; additionally 'val/his_<term>' = the eight histogram terms (mean over the
        pairs).  return_images: also the dict of the generated images (fake_SR, fake_RS, ...)."""
        src_inv, ref_inv, src_msk, ref_msk, c = self.get_input(batch, self.first_stage_key)
        if src_msk is None or ref_msk is None:
            raise KeyError(f"validation_losses needs the label maps '{self.src_msk_key}' and '{self.ref_msk_key}' in the batch")
        fake_SR = self.generate_image(src_inv, c, c_type='c_concat_r')
        fake_RS = self.generate_image(ref_inv, c, c_type='c_concat_s')
        real_S, real_R = torch.cat(c['c_concat_s'], 0), torch.cat(c['c_concat_r'], 0)
        images = dict(fake_SR=fake_SR, fake_RS=fake_RS)
        prefix = 'val'
        loss_dict: Dict[str, torch.Tensor] = {}
        loss_background = self.p_loss_background(SR=fake_SR, RS=fake_RS, src_msk=src_msk, ref_msk=ref_msk, S=real_S, R=real_R)
        loss_dict[f'{prefix}/loss_background'] = loss_background
        loss = self.weight_loss_background * loss_background
        if self.weight_loss_makeup > 0:
            loss_makeup, terms = self.p_loss_makeup(SR=fake_SR, RS=fake_RS, src_msk=src_msk, ref_msk=ref_msk, S=real_S, R=real_R,
                                                    return_terms=True)
            loss_dict[f'{prefix}/loss_makeup'] = loss_makeup
            for name in _ms.TERMS:
                loss_dict[f'{prefix}/his_{name}'] = terms[name].mean()
            loss = loss + self.weight_loss_makeup * loss_makeup
        if self.weight_loss_idt > 0:
            images['fake_SS'] = self.generate_image(src_inv, c, c_type='c_concat_s')
            images['fake_RR'] = self.generate_image(ref_inv, c, c_type='c_concat_r')
            loss_idt = self.p_loss_idt(SS=images['fake_SS'], RR=images['fake_RR'], S=real_S, R=real_R)
            loss_dict[f'{prefix}/loss_idt'] = loss_idt
            loss = loss + self.weight_loss_idt * loss_idt
        if self.weight_loss_cycle > 0:
            images['rec_SS'] = self.generate_image(src_inv, c, c_replace=[fake_RS])
            images['rec_RR'] = self.generate_image(ref_inv, c, c_replace=[fake_SR])
            loss_cycle = self.p_loss_cycle(r_S=images['rec_SS'], r_R=images['rec_RR'], S=real_S, R=real_R)
            loss_dict[f'{prefix}/loss_cycle'] = loss_cycle
            loss = loss + self.weight_loss_cycle * loss_cycle
        return (loss, loss_dict, images) if return_images else (loss, loss_dict)

    def shared_step(self, batch, **kwargs):
        raise NotImplementedError('training losses of diffmk/makeups.py:80-245 are outside the sampling hot path')

    p_losses = forward = shared_step
