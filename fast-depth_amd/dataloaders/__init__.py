"""Device-side input preparation for NYU-Depth-v2 (the reference's `dataloaders` package is CPU code on removed SciPy / NumPy APIs and is
not rebuilt; the arithmetic of its validation transform and of its training augmentation is kept, as index maps and float32 blends on the device)."""
