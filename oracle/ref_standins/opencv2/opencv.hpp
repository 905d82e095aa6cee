/* Declared double of <opencv2/opencv.hpp> -- NOT OpenCV.  The reference's scan registration includes the header and
 * uses no OpenCV symbol, so this is empty on purpose. */
#pragma once
