"""Folder-of-images dataset with the reference's item contract {'img': float[3,S,S] in [0,1]}
(datasets/custom_images.py:20-25)."""
from __future__ import annotations

import os

import numpy as np
import torch


class CustomDataset(torch.utils.data.Dataset):
    EXT = (".png", ".jpg", ".jpeg", ".bmp", ".webp")

    def __init__(self, data_root, image_size=512):
        self.files = sorted(os.path.join(data_root, f) for f in os.listdir(data_root) if f.lower().endswith(self.EXT))
        if not self.files:
            raise FileNotFoundError(f"no images under {data_root}")
        self.size = image_size

    def __len__(self):
        return len(self.files)

    @staticmethod
    def load_image(path, image_size=512):
        """One image file -> float32 [3, image_size, image_size] in [0, 1]: the resize every item of the dataset goes through."""
        from PIL import Image
        img = Image.open(path).convert("RGB").resize((image_size, image_size), Image.BILINEAR)
        return torch.from_numpy(np.asarray(img, dtype=np.float32) / 255.0).permute(2, 0, 1).contiguous()

    def __getitem__(self, i):
        return {"img": self.load_image(self.files[i], self.size)}


class AnnotatedImages(CustomDataset):
    """A folder of images with keypoint annotations: the item contract of the reference's test sets, {'img', 'kpts'[, 'visibility']},
    that `eval.evaluate` and the regressors of keypoint_regressor.py work on.  `annotations.json` in the folder:
        {file name: {"kpts": [[row, col], ...] in [0, 1], "visibility": [0 | 1, ...] (optional)}}
    Every image of the folder must be annotated, with the same number of keypoints; either every entry has "visibility" or none."""

    ANNOTATIONS = "annotations.json"

    def __init__(self, data_root, image_size=512):
        import json
        super().__init__(data_root, image_size)
        with open(os.path.join(data_root, self.ANNOTATIONS)) as f:
            notes = json.load(f)
        names = [os.path.basename(f) for f in self.files]
        missing = [n for n in names if n not in notes]
        if missing:
            raise KeyError(f"{self.ANNOTATIONS} has no entry for {missing[:5]}")
        self.kpts = [torch.tensor(notes[n]["kpts"], dtype=torch.float32) for n in names]
        if any(k.dim() != 2 or k.shape != self.kpts[0].shape or k.shape[1] != 2 for k in self.kpts):
            raise ValueError(f"{self.ANNOTATIONS}: every 'kpts' must be [G][2] with one G")
        with_vis = ["visibility" in notes[n] for n in names]
        if any(with_vis) != all(with_vis):
            raise ValueError(f"{self.ANNOTATIONS}: 'visibility' on some entries only")
        self.visibility = [torch.tensor(notes[n]["visibility"], dtype=torch.float32) for n in names] if all(with_vis) else None
        if self.visibility is not None and any(v.shape != self.kpts[0].shape[:1] for v in self.visibility):
            raise ValueError(f"{self.ANNOTATIONS}: every 'visibility' must have one entry per keypoint")

    def __getitem__(self, i):
        item = super().__getitem__(i)
        item["kpts"] = self.kpts[i].clone()
        if self.visibility is not None:
            item["visibility"] = self.visibility[i].clone()
        return item
