"""Two-level VAE with a PixelSNAIL decoder, model_name='pixelcnn' (reference models/PixelCNN.py:9-124): gated-convolutional
encoders and dense latent layers as in models.convHVAE_2level, and a decoder p(x | z1, z2) that is one PixelSNAIL block over
(x, image(z1), image(z2)) -- utils.nn.PixelSNAIL on the kernels of csrc/evae_attn.hip.  Submodule names (= state_dict keys)
and their order follow the reference; binary inputs only (the reference's grey / continuous heads are out of scope)."""
import numpy as np
import torch
import torch.nn as nn

from evae import ops
from models.AbsHModel import BaseHModel
from utils.nn import Conv2d, GatedConv2d, GatedConvStack, GatedDense, NonLinear, PixelSNAIL

_ENCODER_FEATURES = {'freyfaces': 210, 'cifar10': 384, 'svhn': 384}
_ENCODER_FEATURES_DEFAULT = 294          # 28 x 28 inputs: 6 x 7 x 7
_DENSE_WIDTH = 300
_DECODER_CHANNELS = 64

# (out_channels, kernel, stride, padding) of the five gated convolutions of an encoder
_ENCODER_WIDE = ((32, 7, 1, 3), (32, 3, 2, 1), (64, 5, 1, 2), (64, 3, 2, 1), (6, 3, 1, 1))      # q(z2 | x)
_ENCODER_NARROW = ((32, 3, 1, 1), (32, 3, 2, 1), (64, 3, 1, 1), (64, 3, 2, 1), (6, 3, 1, 1))    # x-branch of q(z1 | x, z2)

PIXEL_DECODE_CHUNK_IMAGES = 2048          # images of one launch of the cached sampler: its cache is 1.8 MB per image, about 3.7 GB
IWAE_CHUNK_ROWS = 100                     # rows of one calculate_loss call of the likelihood estimate (reference utils/evaluation.py:84-92)


def _clip(lo, hi):
    return nn.Hardtanh(min_val=lo, max_val=hi)


class VAE(BaseHModel):
    def __init__(self, args):
        super().__init__(args)

    def _conv_stack(self, c_in, table):
        layers = []
        for c_out, k, s, p in table:
            layers.append(GatedConv2d(c_in, c_out, k, s, p))
            c_in = c_out
        return GatedConvStack(*layers)

    def _gaussian_heads(self, prefix, width, zdim):
        setattr(self, prefix + '_mean', NonLinear(width, zdim, activation=None))
        setattr(self, prefix + '_logvar', NonLinear(width, zdim, activation=_clip(-6., 2.)))

    def create_model(self, args):
        if self.args.input_type != 'binary':
            raise NotImplementedError("pixelcnn: only binary inputs run on the HIP path (input_type=%r)" % (self.args.input_type,))
        if tuple(self.args.input_size[1:]) != (28, 28):
            raise NotImplementedError("pixelcnn: the reference builds its PixelSNAIL for 28 x 28 images")
        self.h_size = _ENCODER_FEATURES.get(args.dataset_name, _ENCODER_FEATURES_DEFAULT)
        feat, fc = self.h_size, _DENSE_WIDTH
        colours, n_pix = self.args.input_size[0], int(np.prod(self.args.input_size))
        z1, z2 = self.args.z1_size, self.args.z2_size

        self.q_z_layers = self._conv_stack(colours, _ENCODER_WIDE)
        self._gaussian_heads('q_z', feat, z2)

        self.q_z1_layers_x = self._conv_stack(colours, _ENCODER_NARROW)
        self.q_z1_layers_z2 = nn.Sequential(GatedDense(z2, feat))
        self.q_z1_layers_joint = nn.Sequential(GatedDense(2 * feat, fc))
        self._gaussian_heads('q_z1', fc, z1)

        self.p_z1_layers_z2 = nn.Sequential(GatedDense(z2, fc), GatedDense(fc, fc))
        self._gaussian_heads('p_z1', fc, z1)

        self.p_x_layers_z1 = nn.Sequential(GatedDense(z1, n_pix))
        self.p_x_layers_z2 = nn.Sequential(GatedDense(z2, n_pix))
        # one PixelSNAIL block of four causal residual blocks and the attention, 64 channels throughout
        self.pixelcnn = PixelSNAIL([28, 28], _DECODER_CHANNELS, _DECODER_CHANNELS, 3, 1, 4, _DECODER_CHANNELS)
        self.p_x_mean = Conv2d(_DECODER_CHANNELS, 1, 1, 1, 0, activation=nn.Sigmoid())

    def _decoder_images(self, z1, z2):
        """the two latent images [B, 2 C, H, W] the decoder reads next to x (they do not depend on x)"""
        shape = (-1,) + tuple(self.args.input_size)
        return torch.cat((self.p_x_layers_z1(z1).view(shape), self.p_x_layers_z2(z2).view(shape)), 1)

    def _given_pixels(self, B, x_given, given, device):
        """(x [B, 784] float32, a fresh tensor the sampler may write; given: an int, or an int64 tensor [B] on the device) of a
        completion; (zeros, None) of a generation from nothing"""
        n_pix = int(np.prod(self.args.input_size))
        if x_given is None and given is None:
            return torch.zeros((B, n_pix), device=device), None
        if x_given is None or given is None:
            raise ValueError("pixelcnn_generate: x_given and given go together")
        if x_given.dim() not in (2, 4) or x_given.shape[0] != B or x_given[0].numel() != n_pix:
            raise ValueError("pixelcnn_generate: x_given must hold %d images of %d pixels (got %s)" % (B, n_pix, tuple(x_given.shape)))
        x = x_given.detach().reshape(B, n_pix).to(device=device, dtype=torch.float32).clone()
        if isinstance(given, (int, np.integer)):
            return x, int(given)
        given = torch.as_tensor(given, device=device).to(torch.int64)
        if tuple(given.shape) != (B,):
            raise ValueError("pixelcnn_generate: given must be an int or one int per image (got shape %s for %d images)"
                             % (tuple(given.shape), B))
        return x, given

    def _pixelcnn_sample(self, z1, z2, x_given=None, given=None):
        """pixelcnn_generate's work: (means [B, 784], images [B, 784])"""
        c, hh, ww = self.args.input_size
        n_pix = c * hh * ww
        sampler = getattr(self.args, 'pixelcnn_sampler', 'passes')
        if sampler not in ('passes', 'cached'):
            raise ValueError("pixelcnn_sampler must be 'passes' or 'cached' (got %r)" % (sampler,))
        B = z1.size(0)
        if sampler == 'cached' and not self.training:
            with torch.no_grad():
                latent = self._decoder_images(z1, z2)
                u = torch.rand(B, n_pix, device=z1.device)
                packed = ops.pixel_decode_pack(self.pixelcnn, self.p_x_mean)
                x, given = self._given_pixels(B, x_given, given, z1.device)
                chunk = int(PIXEL_DECODE_CHUNK_IMAGES)
                G = ops.pixel_decode_choose_images(min(B, chunk))
                if B <= chunk:
                    mean, x, _ = ops.pixel_decode(packed, latent, x, u=u, start=given, images_per_block=G)
                    return mean, x
                # One cache of `chunk` images serves every chunk without being zeroed in between: pixel t of the kernel reads cache
                # positions < t only, and a launch over [0, 784) has written each of them itself before it reads it.
                mean = torch.empty((B, n_pix), device=z1.device)
                cache = ops.PixelDecodeCache(chunk, z1.device)
                for s in range(0, B, chunk):
                    e = min(s + chunk, B)
                    start = given[s:e] if isinstance(given, torch.Tensor) else given
                    ops.pixel_decode(packed, latent[s:e], x[s:e], u=u[s:e], start=start, images_per_block=G,
                                     cache=cache.rows(e - s, mean[s:e]))
                return mean, x
        with torch.no_grad():
            x, given = self._given_pixels(B, x_given, given, z1.device)
            x = x.view(B, c, hh, ww)
            latent = self._decoder_images(z1, z2)
            first = 0
            if given is not None:
                given = torch.full((B,), given, dtype=torch.int64, device=z1.device) if isinstance(given, int) else given
                first = min(max(int(given.min()), 0), n_pix) if B > 0 else 0
            mean = None
            for t in range(first, hh * ww):
                i, j = divmod(t, ww)
                h = torch.cat((x[:, :, :i + 1], latent[:, :, :i + 1]), 1)
                mean = self.p_x_mean(self.pixelcnn(h))                             # [B, 1, i + 1, W]
                draw = torch.bernoulli(mean[:, :, i, j]).float()
                if given is not None:
                    draw = torch.where((t >= given).view(-1, 1), draw, x[:, :, i, j])
                x[:, :, i, j] = draw
            if mean is None:                                                       # every pixel was given: their teacher-forced means
                mean = self.p_x_mean(self.pixelcnn(torch.cat((x, latent), 1)))
            return mean.reshape(-1, n_pix), x.reshape(-1, n_pix)

    def pixelcnn_generate(self, z1, z2, x_given=None, given=None):
        """Ancestral sampling, pixel by pixel in raster order (reference :91-120, binary branch): the mean of pixel (i, j)
        given the pixels drawn so far, one Bernoulli draw from it.  Returns the means of the last pass.  The network is causal:
        the means of rows <= i depend on input rows <= i only, so pass (i, j) runs the decoder on the first i + 1 rows; the last
        pass sees every row, and its result is the reference's.

        args.pixelcnn_sampler = 'cached' (default 'passes': the 784 passes described above), in eval mode: the same ancestral sampling in ONE launch
        of evae.ops.pixel_decode, which evaluates one pixel of every layer at a time over cached activations.  It draws its uniforms
        with one torch.rand(B, 784) where the passes call torch.bernoulli 784 times, so equal seeds give different, equally
        distributed images.  The kernel is the eval-mode network: in training mode (self.training) the reference's dropout stays
        active during generation, and the flag is ignored -- the passes run.

        Completion: x_given ([B, 784] or [B, 1, 28, 28], values 0 / 1) with given (an int, or one per image) keeps the first
        `given` raster pixels of every image as they are and draws the rest given them; the means of the kept pixels are the
        teacher-forced ones.  'cached' hands `given` to its launch as the start pixels; the passes keep the given pixels at their
        write and begin at the smallest `given`.

        'cached' lets the library choose the images per workgroup from the batch (ops.pixel_decode_choose_images: 1 up to 256
        images, where the result is bit-identical to a launch of the default kernel; above that the means differ from the
        1-image kernel's at rounding level, because the attention deals 256 / (8 G) lanes to a head and its sum order depends on
        G), and decodes more than PIXEL_DECODE_CHUNK_IMAGES images in chunks over one reused cache.  The uniforms are drawn once for
        the call and G is chosen once, so the images do not depend on the chunk size."""
        return self._pixelcnn_sample(z1, z2, x_given, given)[0]

    def pixelcnn_complete(self, x, keep_rows, N=1, return_samples=False):
        """Image completion: encode x as reconstruct_x does (forward, which draws z1 and z2), repeat every image N times (rows
        b N ... b N + N - 1 belong to image b), keep the first keep_rows rows -- an int, or one per image -- and draw the rest with
        pixelcnn_generate.  Returns the means [B N, 784]; with return_samples also the completed images [B N, 784]."""
        with torch.no_grad():
            _, _, z = self.forward(x)
            B, ww = x.shape[0], self.args.input_size[2]
            z1 = z[0].reshape(-1, self.args.z1_size).repeat_interleave(N, dim=0)
            z2 = z[3].reshape(-1, self.args.z2_size).repeat_interleave(N, dim=0)
            if isinstance(keep_rows, (int, np.integer)):
                given = ww * int(keep_rows)
            else:
                keep_rows = torch.as_tensor(keep_rows, device=x.device).to(torch.int64)
                if tuple(keep_rows.shape) != (B,):
                    raise ValueError("pixelcnn_complete: keep_rows must be an int or one int per image (got shape %s for %d images)"
                                     % (tuple(keep_rows.shape), B))
                given = (ww * keep_rows).repeat_interleave(N, dim=0)
            mean, samples = self._pixelcnn_sample(z1, z2, x.reshape(B, -1).repeat_interleave(N, dim=0), given)
        return (mean, samples) if return_samples else mean

    def importance_sample_losses(self, data, S, exemplars_embedding):
        """-ELBO of S samples per image in calls of IWAE_CHUNK_ROWS rows: the decoder's activations are 64 channels per pixel
        and row, so the S x D expansion of one call of the other models does not fit it"""
        x = data.reshape(data.size(0), -1).repeat_interleave(S, dim=0)
        out = [self.calculate_loss((x[s:s + IWAE_CHUNK_ROWS], None), exemplars_embedding=exemplars_embedding)[0]
               for s in range(0, x.shape[0], IWAE_CHUNK_ROWS)]
        return torch.cat(out, dim=0)

    def forward(self, x):
        return super().forward(x.view(-1, *self.args.input_size))
