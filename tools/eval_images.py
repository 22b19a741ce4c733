"""Score a folder of generated images against a folder of subject images, as the reference's scripts/stable_txt2img.py does with its
evaluation/ classes: CLIP-I and CLIP-T (--clip), DINO (--dino) and the face similarity (--face-recogniser with --detector).  Prints one JSON
line with the scores that were configured.  Checkpoints are local files; nothing is downloaded.

    python tools/eval_images.py --gen DIR --src DIR --prompt TEXT [--clip FILE] [--dino FILE] [--face-recogniser FILE --detector FILE]
                                [--tokenizer DIR] [--max-batch N]"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--gen", required=True, help="folder of generated images")
    ap.add_argument("--src", required=True, help="folder of subject (reference) images")
    ap.add_argument("--prompt", default="", help="the prompt the images were generated from (placeholder stars are stripped); needed for CLIP-T")
    ap.add_argument("--clip", help="CLIP checkpoint (openai ViT-B-32.pt / transformers layout, .pt / .bin / .safetensors)")
    ap.add_argument("--tokenizer", help="a local CLIPTokenizer folder (without it the word-level stand-in is used and CLIP-T is not reported)")
    ap.add_argument("--dino", help="DINO ViT checkpoint (dino_deitsmall16_pretrain.pth or a transformers ViTModel file)")
    ap.add_argument("--face-recogniser", help="insightface IResNet-100 checkpoint (adaface/iresnet.py)")
    ap.add_argument("--detector", help="RetinaFace-R50 checkpoint (adaface/retinaface.py)")
    ap.add_argument("--max-batch", type=int, default=64)
    ap.add_argument("--device", default="cuda:0")
    a = ap.parse_args(argv)
    if bool(a.face_recogniser) != bool(a.detector):
        ap.error("--face-recogniser and --detector go together")
    if not (a.clip or a.dino or a.face_recogniser):
        ap.error("nothing to score with: give --clip, --dino or --face-recogniser with --detector")

    from adaface_dev_amd.evaluation import eval_utils as EU
    gen, src = EU.list_image_files(a.gen), EU.list_image_files(a.src)
    if not gen or not src:
        ap.error(f"no image files in {a.gen if not gen else a.src}")
    out = {"gen": len(gen), "src": len(src)}
    if a.clip:
        tok = None
        if a.tokenizer:
            from transformers import CLIPTokenizer
            tok = CLIPTokenizer.from_pretrained(a.tokenizer, local_files_only=True)
        ev = EU.ImageDirEvaluator(a.device, clip_model=a.clip, tokenizer=tok, max_batch=a.max_batch)
        out["clip_i"] = ev.img_to_img_similarity(src, gen)
        if tok is not None and a.prompt:
            out["clip_t"] = ev.txt_to_img_similarity(a.prompt.replace("*", ""), gen)
    if a.dino:
        out["dino"] = EU.ViTEvaluator(a.device, dino_model=a.dino, max_batch=a.max_batch).img_to_img_similarity(src, gen)
    if a.face_recogniser:
        import torch
        from adaface_dev_amd.adaface.face_align import FaceIDExtractor
        from adaface_dev_amd.adaface.iresnet import iresnet100
        from adaface_dev_amd.adaface.retinaface import RetinaFace, RetinaFaceDetector, load_retinaface_state_dict
        rec, det = iresnet100(), RetinaFace()
        rec.load_state_dict(torch.load(a.face_recogniser, map_location="cpu", weights_only=True), strict=True)
        load_retinaface_state_dict(det, torch.load(a.detector, map_location="cpu", weights_only=True))
        ex = FaceIDExtractor(rec.to(a.device).eval(), RetinaFaceDetector(det.to(a.device).eval()), device=a.device)
        sim, (n_src, n_gen) = EU.FaceSimilarityEvaluator(ex).compare(src, gen)
        out.update(face_sim=sim, faceless_src=n_src, faceless_gen=n_gen)
    print(json.dumps(out))
    return out


if __name__ == "__main__":
    main()
