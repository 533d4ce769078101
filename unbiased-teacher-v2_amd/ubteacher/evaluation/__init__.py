from .coco_eval import COCOBoxEvaluator, coco_box_ap, coco_box_eval
from .coco_eval_device import DeviceCOCOBoxEvaluator
from .evaluator import inference_on_dataset, inference_context

__all__ = ["COCOBoxEvaluator", "DeviceCOCOBoxEvaluator", "coco_box_ap", "coco_box_eval", "inference_on_dataset", "inference_context"]
