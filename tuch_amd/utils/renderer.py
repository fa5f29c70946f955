"""`Renderer` with the constructor and method signatures of the reference's tuch/utils/renderer.py, over the device
rasteriser of tuch_amd/render.py -- no pyrender, trimesh, OpenGL / EGL or torchvision.

    renderer = Renderer(contactlist, focal_length=5000, img_res=224, faces=smpl.faces)
    img = renderer(vertices, camera_translation, image, colverts=[idxs1, idxs2])       # numpy in, numpy [H,W,3] float32 out
    grid = renderer.visualize_tbm(vertices, camera_translation, images, ...)            # the make_grid tensor [3, ., .]

visualize_tbm, visualize_eft and visu_smplifycontactopti render all bodies and all views in ONE batch (the reference makes
one OpenGL round trip per body and view and colours the vertices in a Python loop) and lay the tiles out as
torchvision.utils.make_grid does (render.image_grid).

Geometry, visibility and the contact colours are the reference's; pyrender's physically based look is not emulated (see
tuch_amd/render.py).  Deliberate departures:
  * the caller's ``camera_translation`` is NOT modified.  The reference flips the sign of its x component in place on
    every call (renderer.py:181), so its three views of one body alternate between two cameras; here every view uses
    the camera whose picture coincides with utils/geometry.perspective_projection(vertices, I, camera_translation, f, c);
  * ``cam_type='weak_perspective'`` (the orthographic camera) is not built: ValueError;
  * the matplotlib keypoint panel of visu_smplifycontactopti is not built: ``keypoints`` must be None there.
Opt-in: tuch_amd.compat.install_renderer() makes this module importable as ``tuch.utils.renderer``.
Constructing needs no device; calling does.
"""
from __future__ import annotations

import numpy as np
import torch

from ..render import MeshRenderer, image_grid

_VIEW_OF = {(False, False): 'front', (True, False): 'rot2', (False, True): 'rot3'}


def _device():
    if not torch.cuda.is_available():
        raise RuntimeError('tuch_amd.utils.renderer renders on a HIP device; none is visible (there is no host fallback)')
    return torch.device('cuda', torch.cuda.current_device())


class Renderer:
    """Renderer used for visualizing the SMPL model (signatures of the reference's class)."""

    def __init__(self, contactlist, focal_length=5000, cam_type='perspective', img_res=224, faces=None):
        if cam_type != 'perspective':
            raise ValueError("cam_type=%r is not built (only 'perspective'; 'weak_perspective' is the reference's "
                             "orthographic EFT camera)" % (cam_type,))
        if faces is None:
            raise ValueError('faces is required')
        self.cam_type = cam_type
        self.focal_length = focal_length
        self.camera_center = [img_res // 2, img_res // 2]
        self.faces = faces
        self.contactlist = contactlist
        self.img_res = img_res
        self.mesh_renderer = MeshRenderer(faces, img_res=img_res, focal_length=focal_length,
                                          camera_center=self.camera_center)

    # ------------------------------------------------------------------------------------------------ one batch
    def _colors(self, verts, contact, colverts):
        """[B,V,3] uint8 or None; contact / colverts: one entry per body or None (renderer.py:200-224: colverts first)."""
        b = verts.shape[0]
        colverts = [None] * b if colverts is None else list(colverts)
        contact = [None] * b if contact is None else list(contact)
        by_pairs = [k for k in range(b) if colverts[k] is not None]
        by_regions = [k for k in range(b) if colverts[k] is None and contact[k] is not None]
        if not by_pairs and not by_regions:
            return None
        colors = torch.full((b, verts.shape[1], 3), 230, dtype=torch.uint8, device=verts.device)
        if by_pairs:
            got = self.mesh_renderer.contact_colors(verts[by_pairs].contiguous(), pairs=[colverts[k] for k in by_pairs])
            colors[by_pairs] = got
        if by_regions:
            flags = np.stack([(np.asarray(contact[k].detach().cpu() if torch.is_tensor(contact[k]) else contact[k])
                               == 1).astype(np.uint8).reshape(-1) for k in by_regions])
            got = self.mesh_renderer.contact_colors(verts[by_regions].contiguous(), contact=flags,
                                                    contactlist=self.contactlist)
            colors[by_regions] = got
        return colors

    def _render(self, vertices, camera_translation, views, background, contact=None, colverts=None):
        """[B,n,H,W,3] device tensor."""
        dev = _device()
        verts = torch.as_tensor(vertices, dtype=torch.float32, device=dev)
        cam = torch.as_tensor(camera_translation, dtype=torch.float32, device=dev)
        bg = None if background is None else torch.as_tensor(background, dtype=torch.float32, device=dev).contiguous()
        colors = self._colors(verts, contact, colverts)
        return self.mesh_renderer.render(verts, cam, views=views, colors=colors, background=bg)['image']

    @staticmethod
    def _tiles(images, rendered):
        """images [B,3,H,W] and rendered [B,n,H,W,3] -> [B (1 + n), 3, H, W]: per body its image, then its views."""
        rend = rendered.permute(0, 1, 4, 2, 3).float().cpu()
        return torch.cat([images.float().cpu().unsqueeze(1), rend], 1).reshape(-1, *rend.shape[2:])

    # ------------------------------------------------------------------------------------------------ the reference's methods
    def visualize_tbm(self, vertices, camera_translation, images, keypoints=None,
                      gt_l3_contact=None, gt_vertsincontact_idx={},
                      has_contact_pc=None, has_contact=None):
        b = vertices.shape[0]
        colverts = [None] * b
        if gt_vertsincontact_idx is not None:
            colverts = [gt_vertsincontact_idx[i] if has_contact[i] else None for i in range(b)]
        contact = [None] * b
        if gt_l3_contact is not None:
            contact = [gt_l3_contact[i] if has_contact_pc[i] else None for i in range(b)]
        rendered = self._render(vertices.detach(), camera_translation.detach(), ('front', 'rot2', 'rot3'),
                                images.detach().permute(0, 2, 3, 1), contact, colverts)
        return image_grid(self._tiles(images.detach(), rendered), nrow=4)

    def visualize_eft(self, vertices, camera_translation, images, contact=None, keypoints=None):
        b = vertices.shape[0]
        rendered = self._render(vertices.detach(), camera_translation.detach(), ('front', 'rot2', 'rot3'),
                                images.detach().permute(0, 2, 3, 1),
                                None if contact is None else [contact[i] for i in range(b)], None)
        return image_grid(self._tiles(images.detach(), rendered), nrow=4)

    def visu_smplifycontactopti(self, verticeslist, camera_translation, images,
                                gt_contact_pc, gt_vertsincontact_idx={}, keypoints=None):
        if keypoints is not None:
            raise ValueError('the matplotlib keypoint panel is not built: keypoints must be None')
        b = images.shape[0]
        steps = sorted(set([0, int(len(verticeslist) * 0.5), len(verticeslist) - 1]))
        plotoptilist = [0, int(len(verticeslist) * 0.5), len(verticeslist) - 1]
        colverts = [None] * b
        if gt_vertsincontact_idx is not None:
            # (the reference keeps the previous body's list for a body without an entry: not reproduced)
            colverts = [gt_vertsincontact_idx[i] if i in gt_vertsincontact_idx else None for i in range(b)]
        contact = [gt_contact_pc[i] for i in range(b)]
        bg = images.detach().permute(0, 2, 3, 1)
        verts = torch.cat([verticeslist[j].detach() for j in steps])                     # [len(steps) B, V, 3]
        rep = len(steps)
        rendered = self._render(verts, camera_translation.detach().repeat(rep, 1), ('front', 'rot2'), bg.repeat(rep, 1, 1, 1),
                                contact * rep, colverts * rep)
        rendered = rendered.reshape(rep, b, 2, *rendered.shape[2:])
        # per body: its image, then (front, rot2) of every plotted step (a step index listed once is drawn once)
        per_body = torch.stack([rendered[k] for k in range(rep)], 1).reshape(b, rep * 2, *rendered.shape[3:])
        return image_grid(self._tiles(images.detach(), per_body), nrow=1 + 2 * len(plotoptilist))

    def __call__(self, vertices, camera_translation, image, contact=None,
                 dorot2=False, dorot3=False, colverts=None):
        """vertices [V,3], camera_translation [3] and image [H,W,3] (or None: white) as numpy -> [H,W,3] float32.
        dorot2 and dorot3 together (the reference applies both turns) give R_x(60) after R_y(60) in its frame."""
        if dorot2 and dorot3:
            from ..render import VIEWS
            view = VIEWS['rot3'] @ VIEWS['rot2']
        else:
            view = _VIEW_OF[(bool(dorot2), bool(dorot3))]
        vertices = np.asarray(vertices, np.float32)[None]
        cam = np.array(camera_translation, np.float32, copy=True)[None]
        over_image = image is not None and not (dorot2 or dorot3)
        dev = _device()
        verts = torch.as_tensor(vertices, device=dev)
        bg = torch.as_tensor(np.asarray(image, np.float32)[None], device=dev) if over_image else None
        colors = self._colors(verts, [contact], [colverts])
        out = self.mesh_renderer.render(verts, torch.as_tensor(cam, device=dev), views=(view,), colors=colors,
                                        background=bg, background_views=[over_image])
        return out['image'][0, 0].cpu().numpy()
