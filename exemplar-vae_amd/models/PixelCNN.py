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

    def pixelcnn_generate(self, z1, z2):
        """Ancestral sampling, pixel by pixel in raster order (reference :91-120, binary branch): the mean of pixel (i, j)
        given the pixels drawn so far, one Bernoulli draw from it.  Returns the means of the last pass.  The network is causal:
        the means of rows <= i depend on input rows <= i only, so pass (i, j) runs the decoder on the first i + 1 rows; the last
        pass sees every row, and its result is the reference's.

        args.pixelcnn_sampler = 'cached' (default 'passes': the 784 passes described above), in eval mode: the same ancestral sampling in ONE launch
        of evae.ops.pixel_decode, which evaluates one pixel of every layer at a time over cached activations.  It draws its uniforms
        with one torch.rand(B, 784) where the passes call torch.bernoulli 784 times, so equal seeds give different, equally
        distributed images.  The kernel is the eval-mode network: in training mode (self.training) the reference's dropout stays
        active during generation, and the flag is ignored -- the passes run."""
        c, hh, ww = self.args.input_size
        sampler = getattr(self.args, 'pixelcnn_sampler', 'passes')
        if sampler not in ('passes', 'cached'):
            raise ValueError("pixelcnn_sampler must be 'passes' or 'cached' (got %r)" % (sampler,))
        if sampler == 'cached' and not self.training:
            with torch.no_grad():
                latent = self._decoder_images(z1, z2)
                u = torch.rand(z1.size(0), c * hh * ww, device=z1.device)
                packed = ops.pixel_decode_pack(self.pixelcnn, self.p_x_mean)
                x = torch.zeros((z1.size(0), c * hh * ww), device=z1.device)
                mean, _, _ = ops.pixel_decode(packed, latent, x, u=u)
                return mean
        with torch.no_grad():
            x = torch.zeros((z1.size(0), c, hh, ww), device=z1.device)
            latent = self._decoder_images(z1, z2)
            mean = None
            for i in range(hh):
                for j in range(ww):
                    h = torch.cat((x[:, :, :i + 1], latent[:, :, :i + 1]), 1)
                    mean = self.p_x_mean(self.pixelcnn(h))                         # [B, 1, i + 1, W]
                    x[:, :, i, j] = torch.bernoulli(mean[:, :, i, j]).float()
            return mean.reshape(-1, int(np.prod(self.args.input_size)))

    def importance_sample_losses(self, data, S, exemplars_embedding):
        """-ELBO of S samples per image in calls of IWAE_CHUNK_ROWS rows: the decoder's activations are 64 channels per pixel
        and row, so the S x D expansion of one call of the other models does not fit it"""
        x = data.reshape(data.size(0), -1).repeat_interleave(S, dim=0)
        out = [self.calculate_loss((x[s:s + IWAE_CHUNK_ROWS], None), exemplars_embedding=exemplars_embedding)[0]
               for s in range(0, x.shape[0], IWAE_CHUNK_ROWS)]
        return torch.cat(out, dim=0)

    def forward(self, x):
        return super().forward(x.view(-1, *self.args.input_size))
