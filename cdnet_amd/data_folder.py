"""Paired-file dataset of the reference (data_folder.py:20-110) and the device-side batch pipeline that feeds the train step.

  img_loader(path, num_channels), get_imgs_list(dir_list, post_fix), DataFolder(dir_list, post_fix, num_channels,
  data_transform)                     same names / arguments / pairing rule as the reference (host side, PIL)
  TileBatches(dataset, opt, device, augment=False)
                                      the MI355X input pipeline: crops / flips on the host (cheap), then ONE
                                      cdnet_label_encoding launch per batch makes the 3-class label, the centre-point map and
                                      the centripetal direction classes (the reference does this per sample in DataLoader
                                      workers, seconds per sample: SURVEY 8f.1).  With augment=True the reference's whole
                                      recipe runs on the device (cdnet_amd/augment.py: random_color, flips, random_elastic,
                                      random_chooseAug and random_crop, and random_resize / random_affine / random_rotation
                                      when the transform dict holds them, in one cdnet_augment_batch[_geo] call per batch,
                                      the sources resident there)

Samples leave TileBatches in the layout train_util_dam.train expects: (input f32 [B,3,H,W] - [B,1,H,W] for a one-channel dataset, whose
images are u8 [H,W] -, weight u8 [B,1,H,W],
label i64 [B,1,H,W] in {0,127,255}, point f16 [B,H,W], direction u8 [B,H,W]).  Without `augment` the photometric / elastic
augmentations of the reference (my_transforms_direction.py:155-473) are skipped and logged; crop and flips are drawn with a numpy
RandomState.  Neither path reproduces the reference's random streams (Python random, np.random, albumentations' RandomState over
DataLoader workers): the contract is the same distributions and the same operation for given parameters."""
import os

import numpy as np
import torch

IMG_EXTENSIONS = ('.jpg', '.jpeg', '.png', '.ppm', '.bmp')


def is_image_file(filename):
    return filename.lower().endswith(IMG_EXTENSIONS)


def grey_image(img, path):
    """the image of a grey-scale dataset (in_c = 1) as 8-bit mode L: L stays as it is, P / RGB / RGBA are converted (a grey-scale dataset
    stored in colour); the modes that hold more than eight bits (I, I;16, F) raise a ValueError that names the file - sixteen-bit sources
    are outside this pipeline.  Anything else comes back as it is."""
    mode = getattr(img, 'mode', None)
    if mode in ('P', 'RGB', 'RGBA'):
        return img.convert('L')
    if mode is not None and (mode == 'F' or mode.startswith('I')):
        raise ValueError('{}: mode {} holds more than 8 bits per pixel; one-channel images are read as 8-bit L'.format(path, mode))
    return img


def img_loader(path, num_channels, grey=False):
    """PIL image of a png / jpg, or of the 'inst_map' of a .mat / the array of a .npy (data_folder.py:20-41).  One channel: the file as it
    is - what the weight maps of every dataset are read with; `grey` (the image of a grey-scale dataset, DataFolder's slot 0 with one
    channel): through grey_image."""
    from PIL import Image
    if path.endswith('.mat'):
        import scipy.io as scio
        arr = scio.loadmat(path)['inst_map']
        return Image.fromarray(arr.astype(np.uint8)) if num_channels == 1 else arr
    if path.endswith('.npy'):
        return Image.fromarray(np.load(path).astype(np.uint8))
    img = Image.open(path)
    if num_channels != 1:
        return img.convert('RGB')
    return grey_image(img, path) if grey else img


def get_imgs_list(dir_list, post_fix=None):
    """[(img, img_<post_fix[0]>, img_<post_fix[1]>, ...)] for every image of dir_list[0] that has all its companions
    (data_folder.py:45-73): companion i lives in dir_list[i] and is called '<image stem>_<post_fix[i-1]>'"""
    if len(dir_list) == 0:
        return []
    if len(dir_list) != len(post_fix) + 1:
        raise RuntimeError('Should specify the postfix of each img type except the first input.')
    present = [set(os.listdir(d)) for d in dir_list]
    out = []
    for name in os.listdir(dir_list[0]):
        if not is_image_file(name):
            continue
        stem = os.path.splitext(name)[0]
        item = [os.path.join(dir_list[0], name)]
        for d, names, pf in zip(dir_list[1:], present[1:], post_fix):
            companion = '{:s}_{:s}'.format(stem, pf)
            if companion in names:
                item.append(os.path.join(d, companion))
        if len(item) == len(dir_list):
            out.append(tuple(item))
    return out


class DataFolder(torch.utils.data.Dataset):
    """one input image, one weight map, one target image per item (data_folder.py:78-110).  With a `data_transform` the item
    is transformed, and re-drawn while its label (third tensor) holds a single value (:103-105)."""

    def __init__(self, dir_list, post_fix, num_channels, data_transform=None, loader=img_loader):
        super().__init__()
        if len(dir_list) != len(post_fix) + 1:
            raise RuntimeError('Length of dir_list is different from length of post_fix + 1.')
        if len(dir_list) != len(num_channels):
            raise RuntimeError('Length of dir_list is different from length of num_channels.')
        self.img_list = get_imgs_list(dir_list, post_fix)
        if len(self.img_list) == 0:
            raise RuntimeError('Found 0 image pairs in given directories.')
        self.data_transform, self.num_channels, self.loader = data_transform, num_channels, loader

    def load(self, index):
        out = [self.loader(p, c) for p, c in zip(self.img_list[index], self.num_channels)]
        if self.num_channels[0] == 1:                # a grey-scale dataset: its image as 8-bit L (the weight map's slot is read as ever)
            out[0] = grey_image(out[0], self.img_list[index][0])
        return out

    def __getitem__(self, index):
        sample = self.load(index)
        if self.data_transform is None:
            return sample
        out = self.data_transform(sample)
        while len(torch.unique(out[2])) <= 1:
            out = self.data_transform(sample)
        return out

    def __len__(self):
        return len(self.img_list)


class TileBatches:
    """Epoch iterator over a DataFolder for the device train step.  Per item: random crop of `input_size` (zero / 0-weight padded
    when the image is smaller), random horizontal / vertical flip when the transform dict asks for them; per batch: one
    cdnet_label_encoding launch.  A crop whose label is constant is re-drawn (the DataFolder rule).  A transform without crop and
    flips (the validation transform) yields every image whole and unpadded, in a fixed order with shuffle=False (batch size 1
    unless the images share one size)."""

    SKIPPED = ('random_color', 'random_elastic', 'random_chooseAug', 'random_resize', 'random_affine', 'random_rotation')
    AUGMENTED = ('random_color', 'random_elastic', 'random_chooseAug', 'random_resize', 'random_affine',
                 'random_rotation')                                             # what augment=True adds (cdnet_amd/augment.py)

    def __init__(self, dataset, transform, batch_size, device, seed=0, shuffle=True, drop_last=False, logger=None, augment=False,
                 elastic=None):
        self.ds, self.B, self.dev = dataset, batch_size, device
        self.rs = np.random.RandomState(seed)
        self.shuffle, self.drop_last = shuffle, drop_last
        self.crop = transform.get('random_crop')
        self.hflip, self.vflip = bool(transform.get('horizontal_flip')), bool(transform.get('vertical_flip'))
        self.normalize = transform.get('normalize')
        self.recipe = None
        if augment:
            if not self.crop:
                raise ValueError('augment=True needs a random_crop transform')
            from .augment import Recipe                                          # elastic: elastic_alpha / _sigma / _alpha_affine
            self.recipe = Recipe.from_transform(transform, **(elastic or {}))
        skipped = [k for k in transform if k in self.SKIPPED and not (augment and k in self.AUGMENTED)]
        if skipped and logger is not None:
            logger.info('input pipeline: augmentations {} are not reproduced (parity unpinned); crop / flips / label encoding are'.format(skipped))
        unknown = [k for k in transform if k not in self.SKIPPED + ('random_crop', 'horizontal_flip', 'vertical_flip', 'label_encoding',
                                                                     'to_tensor', 'normalize')]
        if unknown:
            raise NotImplementedError('transforms {} are outside the accelerated input pipeline'.format(unknown))
        self.items = [[np.asarray(im) for im in dataset.load(i)] for i in range(len(dataset))]      # decoded once, kept on the host
        # label kind, as LabelEncoding decides it per image (`label_level_len > 2`, my_transforms_direction.py:713-720): instance-level
        # labels (the reference's <label_dir>/train_ins layout) take the instance branch of the device transform
        kinds = {len(np.unique(it[2] if it[2].ndim == 2 else it[2][:, :, 0])) > 2 for it in self.items}
        if len(kinds) > 1:
            raise ValueError('the label directory mixes instance-level and 3-class label images')
        self.instance_labels = bool(kinds and kinds.pop())
        self.sources = None
        if self.recipe is not None and torch.device(device).type == 'cuda':
            from .augment import Source                                          # uploaded once, resident on the device
            self.sources = [Source(*it, device) for it in self.items]

    def __len__(self):
        n = len(self.items)
        return n // self.B if self.drop_last else -(-n // self.B)

    def _draw(self, img, weight, label):
        H, W = label.shape[:2]
        if self.recipe is not None:
            # the whole recipe on the host (device='cpu'), re-drawn while the label crop holds one value
            from .augment import augment_host, draw_params
            lab0 = label if label.ndim == 2 else label[:, :, 0]
            w0 = weight if weight.ndim == 2 else weight[:, :, 0]
            for _ in range(50):
                out = augment_host(img, w0, lab0, draw_params(self.rs, H, W, self.recipe), self.recipe.size)
                if len(np.unique(out[2])) > 1:
                    break
            return out
        if not self.crop and not self.hflip and not self.vflip:
            # the reference's validation transform {label_encoding, to_tensor, normalize} (options.py:358): the whole image, untouched -
            # validate() then takes it whole or through split_forward_dam (train_util_dam.py:474)
            return [np.ascontiguousarray(a) for a in (img, weight, label)]
        s = self.crop or max(H, W)
        for _ in range(50):
            y0 = self.rs.randint(0, max(H - s, 0) + 1)
            x0 = self.rs.randint(0, max(W - s, 0) + 1)
            sl = (slice(y0, y0 + s), slice(x0, x0 + s))
            out = [a[sl] for a in (img, weight, label)]
            if out[2].shape[0] < s or out[2].shape[1] < s:
                out = [np.pad(a, ((0, s - a.shape[0]), (0, s - a.shape[1])) + ((0, 0),) * (a.ndim - 2)) for a in out]
            if self.hflip and self.rs.rand() < 0.5:
                out = [a[:, ::-1] for a in out]
            if self.vflip and self.rs.rand() < 0.5:
                out = [a[::-1] for a in out]
            lab0 = out[2] if out[2].ndim == 2 else out[2][:, :, 0]
            if len(np.unique(lab0)) > 1:
                break
        return [np.ascontiguousarray(a) for a in out]

    def __iter__(self):
        from .my_transforms_direction import label_encoding_batch
        order = self.rs.permutation(len(self.items)) if self.shuffle else np.arange(len(self.items))
        for b in range(len(self)):
            idx = order[b * self.B:(b + 1) * self.B]
            if self.sources is not None:
                img, weight, lab0 = self._augment_device(idx)
            else:
                img, weight, lab0 = self._host_batch(idx)
            if self.instance_labels:
                from .my_transforms_direction import label_encoding_instances_batch
                l3, point, direction = label_encoding_instances_batch(lab0.to(torch.int32).contiguous())
            else:
                l3, point, direction = label_encoding_batch(lab0.to(torch.uint8).contiguous())
            yield img.contiguous(), weight.to(torch.uint8).unsqueeze(1), l3.to(torch.int64).unsqueeze(1), point, direction

    def _host_batch(self, idx):
        crops = [self._draw(*self.items[i]) for i in idx]
        img = torch.from_numpy(np.stack([c[0] for c in crops])).to(self.dev)
        img = (img.unsqueeze(1) if img.dim() == 3 else img.permute(0, 3, 1, 2)).float().div(255)        # [H, W] images: one channel
        if self.normalize:
            nc = img.shape[1]
            mean, std = (torch.tensor(v[:nc], device=self.dev).view(1, nc, 1, 1) for v in self.normalize)      # the first in_c entries
            img = (img - mean) / std
        weight = torch.from_numpy(np.stack([c[1] if c[1].ndim == 2 else c[1][:, :, 0] for c in crops])).to(self.dev)
        lab0 = torch.from_numpy(np.stack([c[2] if c[2].ndim == 2 else c[2][:, :, 0] for c in crops])).to(self.dev)
        return img, weight, lab0

    def _augment_device(self, idx):
        """one cdnet_augment_batch call for the batch; samples whose label crop holds one value are re-drawn and re-run together, up to
        50 tries in all (the DataFolder rule)"""
        from .augment import augment_batch, draw_params
        srcs = [self.sources[i] for i in idx]
        draw = lambda s: draw_params(self.rs, s.H, s.W, self.recipe)
        img, weight, lab0, varied = augment_batch(srcs, [draw(s) for s in srcs], self.recipe.size, self.normalize)
        redo = [k for k, v in enumerate(varied.tolist()) if v == 0]
        for _ in range(49):
            if not redo:
                break
            r = augment_batch([srcs[k] for k in redo], [draw(srcs[k]) for k in redo], self.recipe.size, self.normalize)
            sel = torch.tensor(redo, device=img.device)
            img[sel], weight[sel], lab0[sel] = r[0], r[1], r[2]
            redo = [k for k, v in zip(redo, r[3].tolist()) if v == 0]
        return img, weight, lab0
